"""The adversarial discriminator of the 3-D nets on hand-written gfx950 kernels (csrc/adversarial.hip).

``FC3DDiscriminator(num_classes, ndf=64, n_channel=1)`` is the reference's (code/networks/discriminator.py:6-55): same
constructor, same twelve state_dict entries (``conv0`` .. ``conv4`` and ``classifier``, weight and bias each), torch's default
initialisation.  Five Conv3d(kernel 4, stride 2, padding 1), LeakyReLU(0.2) after each, Dropout3d(0.5) after the first three,
AvgPool3d over the 6^3 feature, Linear(8 ndf, 2).  ``pool`` (keyword only, for tests) is another pool window; it has to equal
conv4's output extent.

It is no segmenter: two inputs and a scalar out.  It keeps HipNet's flat parameter and gradient buffers and the nn.Module
surface, and runs its own static launch sequence instead of a Plan:

  ``loss_forward(logits, image, target)``   cross_entropy(D(softmax(logits), image), target).  The ``map`` input is the
      student's LOGITS: the first layer reads them through a softmax (conv0 and conv1 are one convolution over
      num_classes + n_channel channels), the probabilities are never stored.  ``self.training`` decides the dropout; the
      keep decisions come from ``step_state`` (Philox) or from ``drop_masks`` = three [N, C] scale arrays.
  ``loss_backward(params=..., dmap=...)``   the parameter gradients into ``flat_grad`` and / or the gradient at the
      softmax output into ``dmap_buffer()`` (a frozen discriminator forms no parameter gradient).

All buffers are static per batch shape, so both calls can be recorded on a launch tape.  ``_K4S2Discriminator`` is the body;
``FC3DDiscriminator`` here and the 2-D ``FCDiscriminator`` in networks/discriminator_2d.py declare their layer law, pool and
head.  The name ``FCDiscriminator`` stays a stub here that says where it lives.
"""
import torch

from mis_hip import ops
from mis_hip.plan import HipNet

SLOPE = 0.2
DROP_P = 0.5
DROP_SALT = 0x80000000 | 0x0AD50000      # channel mode (bit 31, as mis_norm_act_fwd's Dropout3d sites) + the layer's index


class _K4S2Discriminator(HipNet):
    """The body both discriminators share: conv0 + conv1 (one convolution over the two inputs), conv2, conv3, conv4 -- each
    kernel 4, stride 2, padding 1 -- then a pooled head with a Linear to 2 and the cross-entropy.  A subclass declares
    ``ndim_spatial``, ``LAYER_ACT``, ``POOL``, ``HEAD_WINDOWS`` and ``_head_workspace``; its class name stands in the errors."""
    LAYER_ACT = None        # (slope, dropout) after conv0 + conv1, conv2, conv3, conv4; slope 1.0: no activation
    POOL = None             # the default ``pool``
    HEAD_WINDOWS = None     # pool windows the head flattens: the classifier is Linear(8 ndf * HEAD_WINDOWS, 2)

    @classmethod
    def spec(cls, num_classes, ndf=64, n_channel=1):
        """[(state_dict key, shape)] in the reference's order."""
        return cls._declared(num_classes, ndf, n_channel)

    def __init__(self, num_classes, ndf=64, n_channel=1, *, pool=None):
        super().__init__()
        self.num_classes, self.ndf, self.n_channel = int(num_classes), int(ndf), int(n_channel)
        self.pool = tuple(int(p) for p in (self.POOL if pool is None else pool))
        self._layers(self.num_classes, self.ndf, self.n_channel)
        self._materialize()
        self._bufs = {}
        self._cur = None

    def _layers(self, num_classes, ndf, n_channel):
        for name, cin, cout in (("conv0", num_classes, ndf), ("conv1", n_channel, ndf), ("conv2", ndf, 2 * ndf),
                                ("conv3", 2 * ndf, 4 * ndf), ("conv4", 4 * ndf, 8 * ndf)):
            self._conv(name, cout, cin, (4,) * self.ndim_spatial)
        self._linear("classifier", 2, 8 * ndf * self.HEAD_WINDOWS, law="uniform")

    def _build(self, plan):
        raise RuntimeError(f"{type(self).__name__} has no Plan: use loss_forward / loss_backward")

    def forward(self, map, image):
        raise RuntimeError(f"{type(self).__name__} runs through loss_forward(logits, image, target): it reads the student's "
                           "logits (the softmax is on its load path) and ends in the cross-entropy")

    def _head_workspace(self, N, C, feat):
        """The head's workspace for conv4's output [N, C, *feat]; refuses a ``feat`` the head cannot take."""
        raise NotImplementedError

    # ---- static buffers per batch shape
    def _static(self, N, ext):
        key = (N, *ext)
        b = self._bufs.get(key)
        if b is None:
            if any(e % 16 for e in ext):
                raise RuntimeError(f"{type(self).__name__}: input extent {ext} is no multiple of 16 (MIS_ERR_UNSUPPORTED)")
            widths = [self.ndf, 2 * self.ndf, 4 * self.ndf, 8 * self.ndf]
            head = self._head_workspace(N, widths[3], tuple(e // 16 for e in ext))
            new = lambda *s: torch.zeros(s, dtype=torch.float32, device="cuda")
            exts = [tuple(e >> (i + 1) for e in ext) for i in range(4)]
            b = dict(act=[new(N, c, *e) for c, e in zip(widths, exts)], grad=[new(N, c, *e) for c, e in zip(widths, exts)],
                     scale=[new(N, c) for c, (_, drop) in zip(widths, self.LAYER_ACT) if drop],
                     dmap=new(N, self.num_classes, *(1,) * (3 - len(ext)), *ext), head=head, loss=new(1), logits=new(N, 2))
            self._bufs[key] = b
        return b

    def loss_forward(self, logits, image, target):
        """Writes ``loss_buffer()`` [1] and ``logits_buffer()`` [N, 2].  logits [N, num_classes, *extent] (the student's),
        image [N, n_channel, *extent], target [N] int32; batch-strided views are fine, and so are the [N, C, 1, H, W] views of a
        2-D extent."""
        b = self._static(logits.shape[0], tuple(logits.shape[-self.ndim_spatial:]))
        P = self.P
        scales = [None] * 4
        if self.training and self.dropout_enabled:
            for j, i in enumerate(i for i, (_, drop) in enumerate(self.LAYER_ACT) if drop):
                if self.drop_masks is not None:
                    b["scale"][j].copy_(self.drop_masks[j])
                else:
                    if self.step_state is None:
                        raise RuntimeError(f"{type(self).__name__} in train mode needs step_state (Philox) or drop_masks")
                    ops.channel_dropout_scale(b["scale"][j], DROP_P, DROP_SALT + 16 * self.rng_stream + i, self.step_state)
                scales[i] = b["scale"][j]
        a = b["act"]
        ops.conv_k4s2_fwd(image, logits, P("conv1.weight").data, P("conv0.weight").data, P("conv1.bias").data,
                          P("conv0.bias").data, a[0], self.LAYER_ACT[0][0], scales[0])
        for i, name in ((1, "conv2"), (2, "conv3"), (3, "conv4")):
            ops.conv_k4s2_fwd(a[i - 1], None, P(name + ".weight").data, None, P(name + ".bias").data, None, a[i],
                              self.LAYER_ACT[i][0], scales[i])
        ops.adv_head_fwd(a[3], P("classifier.weight").data, P("classifier.bias").data, target, b["loss"], b["logits"],
                         b["head"], self.pool)
        self._cur = (b, logits, image, scales)
        return b["loss"]

    def loss_backward(self, params=True, dmap=False):
        """Backward of the last loss_forward: ``params`` writes every parameter gradient into ``flat_grad`` (overwriting),
        ``dmap`` the gradient at softmax(logits) into ``dmap_buffer()``."""
        b, logits, image, scales = self._cur
        P = self.P
        g = b["grad"]
        # a layer without an activation (slope 1.0) hands its gradient on as it stands: no stored output goes to the kernels
        y = [a if slope != 1.0 else None for a, (slope, _) in zip(b["act"], self.LAYER_ACT)]
        slope = [s for s, _ in self.LAYER_ACT]
        cw = P("classifier.weight")
        ops.adv_head_bwd(cw.data, g[3], cw.grad if params else None, P("classifier.bias").grad if params else None, b["head"],
                         self.pool)
        for i, name in ((3, "conv4"), (2, "conv3"), (1, "conv2")):
            w = P(name + ".weight")
            if params:
                ops.conv_k4s2_wgrad(b["act"][i - 1], None, g[i], y[i], w.grad, None, P(name + ".bias").grad, None, slope[i],
                                    scales[i])
            ops.conv_k4s2_dgrad(g[i], y[i], w.data, g[i - 1], slope[i], scales[i])
        if params:
            ops.conv_k4s2_wgrad(image, logits, g[0], y[0], P("conv1.weight").grad, P("conv0.weight").grad,
                                P("conv1.bias").grad, P("conv0.bias").grad, slope[0], scales[0])
        if dmap:
            ops.conv_k4s2_dgrad(g[0], y[0], P("conv0.weight").data, b["dmap"], slope[0], scales[0])

    def loss_buffer(self):
        return self._cur[0]["loss"]

    def logits_buffer(self):
        return self._cur[0]["logits"]

    def dmap_buffer(self):
        return self._cur[0]["dmap"]

    def activations(self):
        """The stored outputs of conv0+conv1, conv2, conv3, conv4 of the last loss_forward, each after its activation (if it
        has one) and dropout."""
        return self._cur[0]["act"]


class FC3DDiscriminator(_K4S2Discriminator):
    """LeakyReLU(0.2) after every layer, Dropout3d after the first three, AvgPool3d over the whole 6^3 feature."""
    ndim_spatial = 3
    LAYER_ACT = ((SLOPE, True), (SLOPE, True), (SLOPE, True), (SLOPE, False))
    POOL = (6, 6, 6)
    HEAD_WINDOWS = 1

    def _head_workspace(self, N, C, feat):
        return ops.adv_head_workspace(N, C, 2)      # a pool that is not ``feat`` is refused by the head's entry point


class FCDiscriminator:
    """The 2-D discriminator (reference code/networks/discriminator.py:58-100) is networks.discriminator_2d.FCDiscriminator;
    this module keeps the 3-D one only."""

    def __init__(self, *args, **kwargs):
        raise NotImplementedError("FCDiscriminator (2-D) is not in this module: import it from networks.discriminator_2d")
