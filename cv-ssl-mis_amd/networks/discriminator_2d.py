"""The adversarial discriminator of the 2-D nets on hand-written gfx950 kernels (csrc/adversarial2d.hip).

``FCDiscriminator(num_classes, ndf=64, n_channel=1)`` is the reference's (code/networks/discriminator.py:58-100): same
constructor, same twelve state_dict entries (``conv0`` .. ``conv4`` and ``classifier``, weight and bias each;
``classifier.weight`` is ``(2, 32 ndf)``), torch's default initialisation.  Five Conv2d(kernel 4, stride 2, padding 1) in the
reference's 2-D order, which is not the 3-D one: NO activation and NO dropout after conv0 + conv1, LeakyReLU(0.2) after conv2,
conv3 and conv4, Dropout2d(0.5) after conv2 and conv3 only; then AvgPool2d((7, 7)) -- stride = window, floor mode: at 256^2
conv4 leaves 16 x 16 and the windows cover its top-left 14 x 14, at 224^2 it leaves 14 x 14 -- the flatten over the 2 x 2
windows (feature index c * 4 + wy * 2 + wx) and Linear(32 ndf, 2).  ``pool`` (keyword only, for tests) is another window; an
input whose conv4 output does not give exactly 2 x 2 windows is refused, the classifier is built for those.

The body is FC3DDiscriminator's (``_K4S2Discriminator`` in networks/discriminator.py); this module declares the 2-D layer law,
pool and head.  ``loss_forward(logits, image, target)`` reads the student's LOGITS (the softmax is on the first layer's load
path), ``loss_backward(params=, dmap=)``, ``loss_buffer`` / ``logits_buffer`` / ``dmap_buffer`` / ``activations``;
``drop_masks`` = two [N, C] scale arrays.  Inputs are ``[N, C, H, W]`` or the ``[N, C, 1, H, W]`` views a 2-D HipNet hands out.
"""
from mis_hip import ops
from networks.discriminator import SLOPE, _K4S2Discriminator



class FCDiscriminator(_K4S2Discriminator):
    ndim_spatial = 2
    LAYER_ACT = ((1.0, False), (SLOPE, True), (SLOPE, True), (SLOPE, False))
    POOL = (7, 7)
    HEAD_WINDOWS = 4

    def _head_workspace(self, N, C, feat):
        fh, fw = feat
        if (fh // self.pool[0], fw // self.pool[1]) != (2, 2):
            raise RuntimeError(f"FCDiscriminator: conv4 leaves {fh} x {fw} of an input of {16 * fh} x {16 * fw}, which "
                               f"AvgPool2d({self.pool}) cuts into {fh // self.pool[0]} x {fw // self.pool[1]} windows; "
                               "Linear(32 ndf, 2) needs 2 x 2")
        return ops.adv_head_workspace(N, C, 2, fh, fw, self.pool)
