"""``python train_adversarial_network_2D_ViT.py ...`` on MI355X: adversarial network training with a SwinUnet segmenter.

Command-line drop-in for the reference's code/train_adversarial_network_2D_ViT.py (same flags / defaults, :33-99, ``--cfg`` /
``--opts`` and the other Swin flags included): the segmenter is ``ViT_seg(config, img_size=args.patch_size,
num_classes=args.num_classes)`` + ``load_from(config)`` as in train_mean_teacher_ViT.py (``--model`` is ignored there too),
the discriminator ``networks.discriminator_2d.FCDiscriminator``, the loop the two-phase HIP step of
``mis_hip.step.AdversarialTrainer``.  Without a ``PRETRAIN_CKPT`` file (it is not part of the reference repository)
training starts from scratch.
"""
import argparse
import os

import torch

parser = argparse.ArgumentParser()
parser.add_argument('--root_path', type=str, default='../data/ACDC', help='Name of Experiment')
parser.add_argument('--exp', type=str, default='ACDC/Adversarial_Network_ViT', help='experiment_name')
parser.add_argument('--model', type=str, default='unet', help='model_name')
parser.add_argument('--max_iterations', type=int, default=30000, help='maximum epoch number to train')
parser.add_argument('--batch_size', type=int, default=24, help='batch_size per gpu')
parser.add_argument('--deterministic', type=int, default=1, help='whether use deterministic training')
parser.add_argument('--base_lr', type=float, default=0.01, help='segmentation network learning rate')
parser.add_argument('--DAN_lr', type=float, default=0.0001, help='DAN learning rate')
parser.add_argument('--patch_size', type=int, nargs=2, default=[224, 224], help='patch size of network input')
parser.add_argument('--seed', type=int, default=1337, help='random seed')
parser.add_argument('--num_classes', type=int, default=4, help='output channel of network')
parser.add_argument('--cfg', type=str, default="../code/configs/swin_tiny_patch4_window7_224_lite.yaml")
parser.add_argument("--opts", default=None, nargs='+')
parser.add_argument('--zip', action='store_true')
parser.add_argument('--cache-mode', type=str, default='part', choices=['no', 'full', 'part'])
parser.add_argument('--resume', help='resume from checkpoint')
parser.add_argument('--accumulation-steps', type=int, help="gradient accumulation steps")
parser.add_argument('--use-checkpoint', action='store_true')
parser.add_argument('--amp-opt-level', type=str, default='O1', choices=['O0', 'O1', 'O2'])
parser.add_argument('--tag', help='tag of experiment')
parser.add_argument('--eval', action='store_true')
parser.add_argument('--throughput', action='store_true')
# label and unlabel
parser.add_argument('--labeled_bs', type=int, default=12, help='labeled_batch_size per gpu')
parser.add_argument('--labeled_num', type=int, default=7, help='labeled data')
# costs
parser.add_argument('--ema_decay', type=float, default=0.99, help='ema_decay')
parser.add_argument('--consistency_type', type=str, default="mse", help='consistency_type')
parser.add_argument('--consistency', type=float, default=0.1, help='consistency')
parser.add_argument('--consistency_rampup', type=float, default=200.0, help='consistency_rampup')


def main(argv=None):
    args = parser.parse_args(argv)
    from config import get_config
    from mis_hip.train_common import run_adversarial
    from networks.discriminator_2d import FCDiscriminator
    from networks.vision_transformer import SwinUnet as ViT_seg
    config = get_config(args)
    if config.MODEL.PRETRAIN_CKPT is not None and not os.path.exists(config.MODEL.PRETRAIN_CKPT):
        config.MODEL.PRETRAIN_CKPT = None
    if list(args.patch_size) != [config.DATA.IMG_SIZE] * 2:
        raise SystemExit(f"--patch_size {args.patch_size} != DATA.IMG_SIZE {config.DATA.IMG_SIZE} "
                         "(SwinUnet with window 7 runs at 224; use --opts DATA.IMG_SIZE ...)")

    def make_model():
        net = ViT_seg(config, img_size=args.patch_size, num_classes=args.num_classes).cuda()
        net.load_from(config)
        return net

    args.model = "ViT_Seg" if args.model == "unet" else args.model
    return run_adversarial(args, make_model, lambda: FCDiscriminator(num_classes=args.num_classes), label_dtype=torch.uint8)


if __name__ == "__main__":
    print(main())
