"""``python train_Contrastive_Cross_CNN_ViT_2D.py ...`` on MI355X.

Command-line drop-in for the reference's code/train_Contrastive_Cross_CNN_ViT_2D.py (the flags and defaults of
train_Contrastive_Cross_CNN_2D.py): model1 = ``net_factory(args.model)`` (UNet), model2 = ``ViT_seg(config, ...)`` +
``load_from`` (:139-141), both at ``--patch_size`` 224x224 -- or at 256x256 with ``--patch_size 256 256 --opts
DATA.IMG_SIZE 256 MODEL.SWIN.WINDOW_SIZE 8``.  The loop body is the same fused step, mis_hip.step.ContrastiveCrossTrainer:
only the CNN student receives the contrastive gradient; the Transformer's logits are the key side of both terms.
"""
import os

from train_Contrastive_Cross_CNN_2D import parser


def main(argv=None):
    args = parser.parse_args(argv)
    from mis_hip.step import contrastive_split
    contrastive_split(args.batch_size, args.labeled_bs)      # an odd --labeled_bs is refused before any device work
    from config import get_config
    from mis_hip.train_common import run_contrastive_cross
    from networks.net_factory import net_factory
    from networks.vision_transformer import SwinUnet as ViT_seg
    config = get_config(args)
    if config.MODEL.PRETRAIN_CKPT is not None and not os.path.exists(config.MODEL.PRETRAIN_CKPT):
        config.MODEL.PRETRAIN_CKPT = None
    if list(args.patch_size) != [config.DATA.IMG_SIZE] * 2:
        raise SystemExit(f"--patch_size {args.patch_size} != DATA.IMG_SIZE {config.DATA.IMG_SIZE}: both networks run at "
                         "the SwinUnet's image size (224 with window 7; 256 needs --opts DATA.IMG_SIZE 256 "
                         "MODEL.SWIN.WINDOW_SIZE 8)")

    def make_model1():
        net = net_factory(net_type=args.model, in_chns=1, class_num=args.num_classes)
        if net is None:
            raise SystemExit(f"unknown --model {args.model}")
        return net

    def make_model2():
        net = ViT_seg(config, img_size=args.patch_size, num_classes=args.num_classes).cuda()
        net.load_from(config)
        return net

    return run_contrastive_cross(args, make_model1, make_model2)


if __name__ == "__main__":
    print(main())
