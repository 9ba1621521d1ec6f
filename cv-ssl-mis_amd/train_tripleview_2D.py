"""``python train_tripleview_2D.py ...`` on MI355X.

Command-line drop-in for the reference's ``code/train_tripleview_2D(demo).py`` (the file name without its parentheses): same
flag names and defaults (:43-103: ``--exp ACDC/Triple_View --batch_size 16 --labeled_bs 8 --labeled_num 7``), ``--patch_size``
takes two ints.  model1 and model2 are both ``net_factory(args.model, 1, num_classes)`` with their default initialisation
(:218-220), model3 is ``ViT_seg(config, img_size=args.patch_size, num_classes=args.num_classes)`` + ``load_from(config)``
(:223-225); the loop body (:290-354) runs as mis_hip.step.TripleViewTrainer.  The Swin-specific flags (--cfg/--opts/...) feed
``config.get_config``.
"""
import argparse
import os

parser = argparse.ArgumentParser()
parser.add_argument('--root_path', type=str, default='../data/ACDC', help='Name of Experiment')
parser.add_argument('--exp', type=str, default='ACDC/Triple_View', help='experiment_name')
parser.add_argument('--model', type=str, default='unet', help='model_name')
parser.add_argument('--max_iterations', type=int, default=30000, help='maximum epoch number to train')
parser.add_argument('--batch_size', type=int, default=16, help='batch_size per gpu')
parser.add_argument('--deterministic', type=int, default=1, help='whether use deterministic training')
parser.add_argument('--base_lr', type=float, default=0.01, help='segmentation network learning rate')
parser.add_argument('--patch_size', type=int, nargs=2, default=[224, 224], help='patch size of network input')
parser.add_argument('--seed', type=int, default=1337, help='random seed')
parser.add_argument('--num_classes', type=int, default=4, help='output channel of network')
parser.add_argument('--cfg', type=str, default="../code/configs/swin_tiny_patch4_window7_224_lite.yaml",
                    help='path to config file')
parser.add_argument("--opts", default=None, nargs='+', help="Modify config options by adding 'KEY VALUE' pairs. ")
parser.add_argument('--zip', action='store_true', help='use zipped dataset instead of folder dataset')
parser.add_argument('--cache-mode', type=str, default='part', choices=['no', 'full', 'part'],
                    help='no: no cache, full: cache all data, part: sharding the dataset into nonoverlapping pieces '
                         'and only cache one piece')
parser.add_argument('--resume', help='resume from checkpoint')
parser.add_argument('--accumulation-steps', type=int, help="gradient accumulation steps")
parser.add_argument('--use-checkpoint', action='store_true', help="whether to use gradient checkpointing to save memory")
parser.add_argument('--amp-opt-level', type=str, default='O1', choices=['O0', 'O1', 'O2'],
                    help='mixed precision opt level, if O0, no amp is used')
parser.add_argument('--tag', help='tag of experiment')
parser.add_argument('--eval', action='store_true', help='Perform evaluation only')
parser.add_argument('--throughput', action='store_true', help='Test throughput only')
# label and unlabel
parser.add_argument('--labeled_bs', type=int, default=8, help='labeled_batch_size per gpu')
parser.add_argument('--labeled_num', type=int, default=7, help='labeled data')
# costs
parser.add_argument('--ema_decay', type=float, default=0.99, help='ema_decay')
parser.add_argument('--consistency_type', type=str, default="mse", help='consistency_type')
parser.add_argument('--consistency', type=float, default=0.1, help='consistency')
parser.add_argument('--consistency_rampup', type=float, default=200.0, help='consistency_rampup')


def main(argv=None):
    args = parser.parse_args(argv)
    from mis_hip.step import triple_split
    triple_split(args.batch_size, args.labeled_bs)
    from config import get_config
    from mis_hip.train_common import run_triple_view
    from networks.net_factory import net_factory
    from networks.vision_transformer import SwinUnet as ViT_seg
    config = get_config(args)
    if config.MODEL.PRETRAIN_CKPT is not None and not os.path.exists(config.MODEL.PRETRAIN_CKPT):
        config.MODEL.PRETRAIN_CKPT = None
    if list(args.patch_size) != [config.DATA.IMG_SIZE] * 2:
        raise SystemExit(f"--patch_size {args.patch_size} != DATA.IMG_SIZE {config.DATA.IMG_SIZE}: all three networks run "
                         "at the SwinUnet's image size (224 with window 7; 256 needs --opts DATA.IMG_SIZE 256 "
                         "MODEL.SWIN.WINDOW_SIZE 8)")

    def make_cnn():
        return net_factory(net_type=args.model, in_chns=1, class_num=args.num_classes)

    def make_vit():
        net = ViT_seg(config, img_size=args.patch_size, num_classes=args.num_classes).cuda()
        net.load_from(config)
        return net

    return run_triple_view(args, (make_cnn, make_cnn, make_vit))


if __name__ == "__main__":
    print(main())
