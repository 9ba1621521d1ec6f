"""``net_factory(net_type, in_chns, class_num)`` -- the reference's 2-D model factory surface.

Mirrors code/networks/net_factory.py:77-107: same signature, same key strings, modules are
returned already on the device, unknown keys return ``None``.  Differences, on purpose:
* importing this module does NOT parse ``sys.argv`` (the reference runs a module-level argparse
  and loads a yaml at import, net_factory.py:13-74); ``ViT_Seg`` therefore takes its Swin
  configuration from ``net_factory.swin_config`` (default: the reference's lite yaml with
  ``PRETRAIN_CKPT=None``) instead of module-level ``args``/``config`` globals;
* ``unet`` and ``ViT_Seg`` are on the hand-written HIP hot path, and so are ``classifier`` and ``projector``, the frozen
  heads of the contrastive cross-teaching scripts (networks/projector.py; built with their defaults, as in the reference),
  and ``pnet`` (networks/pnet.py: ``PNet2D(in_chns, class_num, 64, [1, 2, 4, 8, 16])``, its dilated 3x3 convolutions on
  csrc/conv_dilated.hip).
  The other keys of the reference (enet, unet_ds, unet_cct, unet_urpc, efficient_unet, nnUNet, preunet) belong to
  other SSL methods / backbones that SURVEY.md s.8 marks out of scope; they raise ``NotImplementedError`` naming the
  scope decision instead of silently returning something else.
"""
from config import lite_config
from networks.pnet import PNet2D
from networks.projector import classifier, projectors
from networks.unet import UNet
from networks.vision_transformer import SwinUnet as ViT_seg

_OUT_OF_SCOPE = ("enet", "unet_ds", "unet_cct", "unet_urpc", "efficient_unet", "nnUNet", "preunet")

swin_config = None   # set to a config.get_config(args) result to override the lite defaults


def net_factory(net_type="unet", in_chns=1, class_num=3):
    if net_type == "unet":
        net = UNet(in_chns=in_chns, class_num=class_num).cuda()
    elif net_type == "ViT_Seg":
        cfg = swin_config if swin_config is not None else lite_config()
        net = ViT_seg(cfg, img_size=cfg.DATA.IMG_SIZE, num_classes=class_num).cuda()
    elif net_type == "pnet":
        net = PNet2D(in_chns, class_num, 64, [1, 2, 4, 8, 16]).cuda()
    elif net_type == "classifier":
        net = classifier().cuda()
    elif net_type == "projector":
        net = projectors().cuda()
    elif net_type in _OUT_OF_SCOPE:
        raise NotImplementedError(
            f"net_type '{net_type}' is a valid reference key but outside the Mean-Teacher hot path built here "
            "(SURVEY.md s.8: other backbones / SSL methods are out of scope)")
    else:
        net = None
    return net
