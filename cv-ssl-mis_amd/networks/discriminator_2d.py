"""The adversarial discriminator of the 2-D nets on hand-written gfx950 kernels (csrc/adversarial2d.hip).

``FCDiscriminator(num_classes, ndf=64, n_channel=1)`` is the reference's (code/networks/discriminator.py:58-100): same
constructor, same twelve state_dict entries (``conv0`` .. ``conv4`` and ``classifier``, weight and bias each;
``classifier.weight`` is ``(2, 32 ndf)``), torch's default initialisation.  Five Conv2d(kernel 4, stride 2, padding 1) in the
reference's 2-D order, which is not the 3-D one: NO activation and NO dropout after conv0 + conv1, LeakyReLU(0.2) after conv2,
conv3 and conv4, Dropout2d(0.5) after conv2 and conv3 only; then AvgPool2d((7, 7)) -- stride = window, floor mode: at 256^2
conv4 leaves 16 x 16 and the windows cover its top-left 14 x 14, at 224^2 it leaves 14 x 14 -- the flatten over the 2 x 2
windows (feature index c * 4 + wy * 2 + wx) and Linear(32 ndf, 2).  ``pool`` (keyword only, for tests) is another window; an
input whose conv4 output does not give exactly 2 x 2 windows is refused, the classifier is built for those.

The interface is FC3DDiscriminator's (networks/discriminator.py): ``loss_forward(logits, image, target)`` reads the student's
LOGITS (the softmax is on the first layer's load path), ``loss_backward(params=, dmap=)``, ``loss_buffer`` / ``logits_buffer``
/ ``dmap_buffer`` / ``activations``; ``drop_masks`` = two [N, C] scale arrays.  Inputs are ``[N, C, H, W]`` or the
``[N, C, 1, H, W]`` views a 2-D HipNet hands out.  All buffers are static per batch shape: both calls can be recorded on a
launch tape.
"""
import torch

from mis_hip import ops
from mis_hip.plan import HipNet
from networks.discriminator import DROP_P, DROP_SALT, SLOPE

# (slope, dropout) after conv0 + conv1, conv2, conv3, conv4
LAYER_ACT = ((1.0, False), (SLOPE, True), (SLOPE, True), (SLOPE, False))


class FCDiscriminator(HipNet):
    ndim_spatial = 2

    @classmethod
    def spec(cls, num_classes, ndf=64, n_channel=1):
        """[(state_dict key, shape)] in the reference's order."""
        return cls._declared(num_classes, ndf, n_channel)

    def __init__(self, num_classes, ndf=64, n_channel=1, *, pool=(7, 7)):
        super().__init__()
        self.num_classes, self.ndf, self.n_channel = int(num_classes), int(ndf), int(n_channel)
        self.pool = tuple(int(p) for p in pool)
        self._layers(self.num_classes, self.ndf, self.n_channel)
        self._materialize()
        self._bufs = {}
        self._cur = None

    def _layers(self, num_classes, ndf, n_channel):
        for name, cin, cout in (("conv0", num_classes, ndf), ("conv1", n_channel, ndf), ("conv2", ndf, 2 * ndf),
                                ("conv3", 2 * ndf, 4 * ndf), ("conv4", 4 * ndf, 8 * ndf)):
            self._conv(name, cout, cin, (4, 4))
        self._linear("classifier", 2, 32 * ndf, law="uniform")

    def _build(self, plan):
        raise RuntimeError("FCDiscriminator has no Plan: use loss_forward / loss_backward")

    def forward(self, map, feature):
        raise RuntimeError("FCDiscriminator runs through loss_forward(logits, image, target): it reads the student's logits "
                           "(the softmax is on its load path) and ends in the cross-entropy")

    # ---- static buffers per batch shape
    def _static(self, N, H, W):
        key = (N, H, W)
        b = self._bufs.get(key)
        if b is None:
            if H % 16 or W % 16:
                raise RuntimeError(f"FCDiscriminator: input extent {(H, W)} is no multiple of 16 (MIS_ERR_UNSUPPORTED)")
            fh, fw = H // 16, W // 16
            if (fh // self.pool[0], fw // self.pool[1]) != (2, 2):
                raise RuntimeError(f"FCDiscriminator: conv4 leaves {fh} x {fw} of an input of {H} x {W}, which AvgPool2d({self.pool}) "
                                   f"cuts into {fh // self.pool[0]} x {fw // self.pool[1]} windows; Linear(32 ndf, 2) needs 2 x 2")
            new = lambda *s: torch.zeros(s, dtype=torch.float32, device="cuda")
            widths = [self.ndf, 2 * self.ndf, 4 * self.ndf, 8 * self.ndf]
            ext = [(H >> (i + 1), W >> (i + 1)) for i in range(4)]
            b = dict(act=[new(N, c, *e) for c, e in zip(widths, ext)], grad=[new(N, c, *e) for c, e in zip(widths, ext)],
                     scale=[new(N, c) for c in widths[1:3]], dmap=new(N, self.num_classes, 1, H, W),
                     head=ops.adv_head2d_workspace(N, widths[3], 2, fh, fw, self.pool), loss=new(1), logits=new(N, 2))
            self._bufs[key] = b
        return b

    def loss_forward(self, logits, image, target):
        """Writes ``loss_buffer()`` [1] and ``logits_buffer()`` [N, 2].  logits [N, num_classes, (1,) H, W] (the student's),
        image [N, n_channel, (1,) H, W], target [N] int32; batch-strided views are fine."""
        N, H, W = logits.shape[0], logits.shape[-2], logits.shape[-1]
        b = self._static(N, H, W)
        P = self.P
        scales = [None, None, None, None]
        if self.training and self.dropout_enabled:
            for j, i in enumerate((1, 2)):
                if self.drop_masks is not None:
                    b["scale"][j].copy_(self.drop_masks[j])
                else:
                    if self.step_state is None:
                        raise RuntimeError("FCDiscriminator in train mode needs step_state (Philox) or drop_masks")
                    ops.channel_dropout_scale(b["scale"][j], DROP_P, DROP_SALT + 16 * self.rng_stream + i, self.step_state)
                scales[i] = b["scale"][j]
        a = b["act"]
        ops.conv2d_k4s2_fwd(image, logits, P("conv1.weight").data, P("conv0.weight").data, P("conv1.bias").data,
                            P("conv0.bias").data, a[0], 1.0, None)
        for i, name in ((1, "conv2"), (2, "conv3"), (3, "conv4")):
            ops.conv2d_k4s2_fwd(a[i - 1], None, P(name + ".weight").data, None, P(name + ".bias").data, None, a[i],
                                LAYER_ACT[i][0], scales[i])
        ops.adv_head2d_fwd(a[3], P("classifier.weight").data, P("classifier.bias").data, target, b["loss"], b["logits"],
                           b["head"], self.pool)
        self._cur = (b, logits, image, scales)
        return b["loss"]

    def loss_backward(self, params=True, dmap=False):
        """Backward of the last loss_forward: ``params`` writes every parameter gradient into ``flat_grad`` (overwriting),
        ``dmap`` the gradient at softmax(logits) into ``dmap_buffer()``."""
        b, logits, image, scales = self._cur
        P = self.P
        a, g = b["act"], b["grad"]
        cw = P("classifier.weight")
        ops.adv_head2d_bwd(cw.data, g[3], cw.grad if params else None, P("classifier.bias").grad if params else None,
                           b["head"], self.pool)
        for i, name in ((3, "conv4"), (2, "conv3"), (1, "conv2")):
            w = P(name + ".weight")
            if params:
                ops.conv2d_k4s2_wgrad(a[i - 1], None, g[i], a[i], w.grad, None, P(name + ".bias").grad, None, SLOPE, scales[i])
            ops.conv2d_k4s2_dgrad(g[i], a[i], w.data, g[i - 1], SLOPE, scales[i])
        # conv0 + conv1 carry no activation: their gradient is g[0] as it stands
        if params:
            ops.conv2d_k4s2_wgrad(image, logits, g[0], None, P("conv1.weight").grad, P("conv0.weight").grad,
                                  P("conv1.bias").grad, P("conv0.bias").grad, 1.0, None)
        if dmap:
            ops.conv2d_k4s2_dgrad(g[0], None, P("conv0.weight").data, b["dmap"], 1.0, None)

    def loss_buffer(self):
        return self._cur[0]["loss"]

    def logits_buffer(self):
        return self._cur[0]["logits"]

    def dmap_buffer(self):
        return self._cur[0]["dmap"]

    def activations(self):
        """The stored outputs of conv0+conv1 (not activated), conv2, conv3, conv4 of the last loss_forward."""
        return self._cur[0]["act"]
