"""The contrastive heads (``net_factory("projector" | "classifier")``) on hand-written gfx950 kernels.

Drop-ins for the reference's ``networks.projector.projectors`` and ``classifier`` (code/networks/projector.py:50-92): same
constructor defaults, same ``forward``, same state_dict keys and shapes -- ``conv_{i}.conv.{weight,bias}``,
``conv_{i}.bn.{weight,bias,running_mean,running_var,num_batches_tracked}``, ``final.{weight,bias}`` -- and torch's default
initialisation.  Each block is ``Conv2d(3x3, padding 1) -> BatchNorm2d -> ReLU -> MaxPool2d(2)``: two of them in the
projector (C -> 8 -> 16 channels at a quarter of the resolution), three in the classifier (-> 32 at an eighth) followed by
its 1x1 ``final`` convolution.  ``projectors.final`` is declared and never called by the reference's forward; it is a
state_dict key here too and no op reads it.

The contrastive cross-teaching scripts put these heads in no optimizer: they stay as initialised, in train mode (BatchNorm
normalises with the statistics of the sub-batch it sees and updates its running buffers), and a backward through them
needs the gradient at their INPUT -- the students' logits -- and nothing else.  Hence ``frozen = True`` (mis_hip.plan:
no weight, bias or affine gradient launch, filters packed once), a first convolution built with ``need_dx=True``, and
``input_grad_buffer()`` to read the result.  ``strided_input``: the classifier's input ``logits[:L][0::2]`` is bound as
the batch-strided view it is.
"""
from mis_hip.plan import HipNet


class _Head(HipNet):
    ndim_spatial = 2
    frozen = True
    strided_input = True
    BLOCKS = 0              # conv_1 .. conv_BLOCKS
    CALLS_FINAL = False

    @classmethod
    def spec(cls, in_chns=4, ndf=8):
        """[(state_dict key, shape)] in the reference's order."""
        return cls._declared([int(in_chns)] + [int(ndf) << i for i in range(cls.BLOCKS)])

    def __init__(self, in_chns, ndf):
        super().__init__()
        self.in_chns, self.ndf = int(in_chns), int(ndf)
        self.widths = [self.in_chns] + [self.ndf << i for i in range(self.BLOCKS)]
        self._layers(self.widths)
        self._materialize()

    def _layers(self, widths):
        for i in range(1, len(widths)):
            self._conv(f"conv_{i}.conv", widths[i], widths[i - 1], (3, 3))
            self._norm(f"conv_{i}.bn", widths[i], running=True)
        self._conv("final", widths[-1], widths[-1], (1, 1))

    @property
    def out_channels(self):
        return self.widths[-1]

    def _build(self, plan):
        N, C, D, H, W = plan.in_shape
        div = 1 << self.BLOCKS
        if C != self.in_chns or D != 1 or H % div or W % div:
            raise RuntimeError(f"{type(self).__name__} input must be [N,{self.in_chns},H,W] with H,W multiples of {div}; "
                               f"got {(N, C, H, W)}")
        P, B = self.P, self.B
        x = plan.inp
        for i in range(1, self.BLOCKS + 1):
            cout = self.widths[i]
            sp = (1, H >> (i - 1), W >> (i - 1))
            t = plan.new(cout, sp)
            # need_dx on the first conv too: the gradient at the head's input is what its backward is for
            plan.conv(x, t, P(f"conv_{i}.conv.weight"), P(f"conv_{i}.conv.bias"), (3, 3), need_dx=True, bias_grad=False)
            y = plan.new(cout, sp)
            plan.norm_act(t, y, per_sample=False, gamma=P(f"conv_{i}.bn.weight"), beta=P(f"conv_{i}.bn.bias"),
                          running=(B(f"conv_{i}.bn.running_mean"), B(f"conv_{i}.bn.running_var"),
                                   B(f"conv_{i}.bn.num_batches_tracked")), slope=0.0)
            # plan.maxpool takes the fused form (pool inside the normalisation's passes) where the geometry allows it
            # (W % 8 forward, W % 4 backward) and the plain pair of launches otherwise
            x = plan.maxpool(y, plan.new(cout, (1, H >> i, W >> i)))
        if self.CALLS_FINAL:
            plan.out = plan.new(self.widths[-1], (1, H >> self.BLOCKS, W >> self.BLOCKS))
            plan.conv(x, plan.out, P("final.weight"), P("final.bias"), (1, 1), bias_grad=True)
        else:
            plan.out = x


class projectors(_Head):
    """reference networks/projector.py:50-67"""
    BLOCKS = 2

    def __init__(self, input_nc=4, ndf=8, norm_layer=None):
        super().__init__(input_nc, ndf)


class classifier(_Head):
    """reference networks/projector.py:69-92"""
    BLOCKS = 3
    CALLS_FINAL = True

    def __init__(self, inp_dim=4, ndf=8, norm_layer=None):
        super().__init__(inp_dim, ndf)
