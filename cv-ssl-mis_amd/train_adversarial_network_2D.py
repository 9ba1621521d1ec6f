"""``python train_adversarial_network_2D.py --model unet ...`` on MI355X.

Command-line drop-in for the reference's code/train_adversarial_network_2D.py: same flag names and defaults (:31-66,
``--DAN_lr`` included).  ``--patch_size`` takes two integers (the reference declares ``type=list``, which only its default
survives).  The hot loop runs as the two-phase HIP step of ``mis_hip.step.AdversarialTrainer``; the discriminator is
``networks.discriminator_2d.FCDiscriminator``.  ``--model`` takes every key ``net_factory`` serves for a segmenter.
``--ema_decay`` and ``--consistency_type`` are parsed and unused, as in the reference.

The reference's script does not parse as it stands (:211, a doubled comma in the validation call): this one mirrors its
loop -- the loop of the 3-D script with ``FCDiscriminator`` and 2-D validation -- not the typo.
"""
import argparse

import torch

parser = argparse.ArgumentParser()
parser.add_argument('--root_path', type=str, default='../data/ACDC', help='Name of Experiment')
parser.add_argument('--exp', type=str, default='ACDC/Adversarial_Network', help='experiment_name')
parser.add_argument('--model', type=str, default='unet', help='model_name')
parser.add_argument('--max_iterations', type=int, default=30000, help='maximum epoch number to train')
parser.add_argument('--batch_size', type=int, default=24, help='batch_size per gpu')
parser.add_argument('--deterministic', type=int, default=1, help='whether use deterministic training')
parser.add_argument('--base_lr', type=float, default=0.01, help='segmentation network learning rate')
parser.add_argument('--DAN_lr', type=float, default=0.0001, help='DAN learning rate')
parser.add_argument('--patch_size', type=int, nargs=2, default=[256, 256], help='patch size of network input')
parser.add_argument('--seed', type=int, default=1337, help='random seed')
parser.add_argument('--num_classes', type=int, default=4, help='output channel of network')
# label and unlabel
parser.add_argument('--labeled_bs', type=int, default=12, help='labeled_batch_size per gpu')
parser.add_argument('--labeled_num', type=int, default=3, help='labeled data')
# costs
parser.add_argument('--ema_decay', type=float, default=0.99, help='ema_decay')
parser.add_argument('--consistency_type', type=str, default="mse", help='consistency_type')
parser.add_argument('--consistency', type=float, default=0.1, help='consistency')
parser.add_argument('--consistency_rampup', type=float, default=200.0, help='consistency_rampup')


def main(argv=None):
    args = parser.parse_args(argv)
    from mis_hip.train_common import run_adversarial
    from networks.discriminator_2d import FCDiscriminator
    from networks.net_factory import net_factory

    def make_model():
        net = net_factory(net_type=args.model, in_chns=1, class_num=args.num_classes)
        if net is None:
            raise SystemExit(f"unknown --model {args.model}")
        return net

    return run_adversarial(args, make_model, lambda: FCDiscriminator(num_classes=args.num_classes), label_dtype=torch.uint8)


if __name__ == "__main__":
    print(main())
