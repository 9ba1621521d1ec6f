"""``python train_interpolation_consistency_training_2D.py --model unet ...`` on MI355X.

Command-line drop-in for the reference's code/train_interpolation_consistency_training_2D.py: same flag names and
defaults (:30-66).  Two flags are parsed differently, because the reference's types cannot take their defaults from a
shell: ``--patch_size`` takes two ints (``type=list`` there) and ``--ict_alpha`` takes a float (``type=int`` there,
with the default 0.2).  The hot loop (:150-190) runs as mis_hip.step.ICTTrainer: device Beta(ict_alpha, ict_alpha)
mix factors, the mixed student input, two teacher forwards and the mixed-target consistency; no ``iter_num < 1000``
gate in this script.  ``batch_size - labeled_bs`` must equal ``2 * (labeled_bs // 2)``.
"""
import argparse

import torch

parser = argparse.ArgumentParser()
parser.add_argument('--root_path', type=str, default='../data/ACDC', help='Name of Experiment')
parser.add_argument('--exp', type=str, default='ACDC/Interpolation_Consistency_Training', help='experiment_name')
parser.add_argument('--model', type=str, default='unet', help='model_name')
parser.add_argument('--max_iterations', type=int, default=30000, help='maximum epoch number to train')
parser.add_argument('--batch_size', type=int, default=24, help='batch_size per gpu')
parser.add_argument('--deterministic', type=int, default=1, help='whether use deterministic training')
parser.add_argument('--base_lr', type=float, default=0.01, help='segmentation network learning rate')
parser.add_argument('--patch_size', type=int, nargs=2, default=[256, 256], help='patch size of network input')
parser.add_argument('--seed', type=int, default=1337, help='random seed')
parser.add_argument('--num_classes', type=int, default=4, help='output channel of network')
# label and unlabel
parser.add_argument('--labeled_bs', type=int, default=12, help='labeled_batch_size per gpu')
parser.add_argument('--labeled_num', type=int, default=300, help='labeled data')
parser.add_argument('--ict_alpha', type=float, default=0.2, help='ict_alpha')
# costs
parser.add_argument('--ema_decay', type=float, default=0.99, help='ema_decay')
parser.add_argument('--consistency_type', type=str, default="mse", help='consistency_type')
parser.add_argument('--consistency', type=float, default=0.1, help='consistency')
parser.add_argument('--consistency_rampup', type=float, default=200.0, help='consistency_rampup')


def main(argv=None):
    args = parser.parse_args(argv)
    from mis_hip.step import ICTTrainer, ict_split
    ict_split(args.batch_size, args.labeled_bs)          # the batch-shape rule, before any device work
    from mis_hip.train_common import run_training
    from networks.net_factory import net_factory

    def make_model():
        net = net_factory(net_type=args.model, in_chns=1, class_num=args.num_classes)
        if net is None:
            raise SystemExit(f"unknown --model {args.model}")
        return net

    return run_training(args, make_model, label_dtype=torch.uint8, cons_start_iter=0, save_ema=False,
                        trainer_cls=ICTTrainer, trainer_kw=dict(ict_alpha=args.ict_alpha))


if __name__ == "__main__":
    print(main())
