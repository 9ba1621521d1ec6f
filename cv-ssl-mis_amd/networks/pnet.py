"""PNet2D (``--model pnet``) on hand-written gfx950 kernels.

Drop-in for the reference's ``networks.pnet.PNet2D`` (code/networks/pnet.py:87-122, the DeepIGeoS P-Net): same
constructor, same ``forward(x[N,C,H,W]) -> logits[N,out_chns,H,W]``, same state_dict keys, order and shapes --
``block{1..5}.{conv1,conv2}.{weight,bias}``, ``block{k}.{in1,in2}.{weight,bias,running_mean,running_var,num_batches_tracked}``,
``catblock.{conv1,conv2}.*``, ``out.{conv1,conv2}.*`` -- and torch's default initialisation.

Five ``PNetBlock``s at full resolution (no pooling): ``Conv2d(3x3, dilation = padding = r_k)`` -> BatchNorm2d ->
LeakyReLU(0.01), twice.  The block outputs are concatenated (``torch.cat`` never runs: every block's second activation is
written straight into its channel slice of one ``[N, 5F, H, W]`` buffer, the next block reads that slice),
``catblock`` is 1x1 -> LeakyReLU -> 1x1 -> LeakyReLU, ``out`` is Dropout2d(0.3) -> 1x1 -> LeakyReLU -> Dropout2d(0.3) -> 1x1.
Each Dropout2d is folded into the activation in front of it (channel-wise dropout of ``mis_norm_act_*`` without a norm).
The convolutions with r_k > 1 run on csrc/conv_dilated.hip, those with r_k = 1 and the 1x1 ones on the dense kernels.

The layer graph is executed by ``mis_hip.plan``; nothing here computes on the CPU.
"""
from mis_hip.plan import HipNet

_SLOPE = 0.01       # nn.LeakyReLU() default
_DROP = 0.3         # OutPutBlock's two nn.Dropout2d


class PNet2D(HipNet):
    ndim_spatial = 2

    @classmethod
    def spec(cls, in_chns, out_chns, num_filters, ratios=(1, 2, 4, 8, 16)):
        """[(state_dict key, shape)] in the reference's order."""
        return cls._declared(in_chns, out_chns, num_filters)

    def __init__(self, in_chns, out_chns, num_filters, ratios):
        super().__init__()
        self.in_chns, self.out_chns, self.num_filters = int(in_chns), int(out_chns), int(num_filters)
        self.ratios = [int(r) for r in ratios]
        if len(self.ratios) != 5:
            raise ValueError(f"PNet2D has five blocks: five dilation ratios expected, got {ratios}")
        self._layers(in_chns, out_chns, num_filters)
        self._materialize()

    def _layers(self, in_chns, out_chns, F):
        for k in range(1, 6):
            self._conv(f"block{k}.conv1", F, in_chns if k == 1 else F, (3, 3))
            self._conv(f"block{k}.conv2", F, F, (3, 3))
            self._norm(f"block{k}.in1", F, running=True)
            self._norm(f"block{k}.in2", F, running=True)
        self._conv("catblock.conv1", 5 * F, 5 * F, (1, 1))
        self._conv("catblock.conv2", 2 * F, 5 * F, (1, 1))
        self._conv("out.conv1", F, 2 * F, (1, 1))
        self._conv("out.conv2", out_chns, F, (1, 1))

    def _bn(self, prefix):
        P, B = self.P, self.B
        return dict(per_sample=False, gamma=P(f"{prefix}.weight"), beta=P(f"{prefix}.bias"),
                    running=(B(f"{prefix}.running_mean"), B(f"{prefix}.running_var"), B(f"{prefix}.num_batches_tracked")),
                    slope=_SLOPE)

    def _build(self, plan):
        N, C, D, H, W = plan.in_shape
        if C != self.in_chns or D != 1:
            raise RuntimeError(f"PNet2D input must be [N,{self.in_chns},H,W]; got {(N, C, H, W) if D == 1 else plan.in_shape}")
        P, F, sp = self.P, self.num_filters, (1, H, W)
        cat = plan.new(5 * F, sp)
        x = plan.inp
        for k in range(1, 6):
            r, b = self.ratios[k - 1], f"block{k}"
            t = plan.new(F, sp)
            # the bias in front of a BatchNorm has an exactly zero gradient (bias_grad=False)
            plan.conv(x, t, P(f"{b}.conv1.weight"), P(f"{b}.conv1.bias"), (3, 3), need_dx=k > 1, bias_grad=False, dilation=r)
            a = plan.norm_act(t, plan.new(F, sp), **self._bn(f"{b}.in1"))
            t = plan.new(F, sp)
            plan.conv(a, t, P(f"{b}.conv2.weight"), P(f"{b}.conv2.bias"), (3, 3), bias_grad=False, dilation=r)
            x = plan.norm_act(t, plan.view(cat, (k - 1) * F, F), **self._bn(f"{b}.in2"))
        # ConcatBlock (pnet.py:45-62)
        t = plan.new(5 * F, sp)
        plan.conv(cat, t, P("catblock.conv1.weight"), P("catblock.conv1.bias"), (1, 1))
        a = plan.norm_act(t, plan.new(5 * F, sp), per_sample=False, slope=_SLOPE, no_norm=True)
        t = plan.new(2 * F, sp)
        plan.conv(a, t, P("catblock.conv2.weight"), P("catblock.conv2.bias"), (1, 1))
        # ... its second LeakyReLU carries OutPutBlock's drop1, out.ac1 carries drop2 (pnet.py:78-84)
        a = plan.norm_act(t, plan.new(2 * F, sp), per_sample=False, slope=_SLOPE, drop_p=_DROP, drop3d=True, no_norm=True)
        t = plan.new(F, sp)
        plan.conv(a, t, P("out.conv1.weight"), P("out.conv1.bias"), (1, 1))
        a = plan.norm_act(t, plan.new(F, sp), per_sample=False, slope=_SLOPE, drop_p=_DROP, drop3d=True, no_norm=True)
        plan.out = plan.new(self.out_chns, sp)
        plan.conv(a, plan.out, P("out.conv2.weight"), P("out.conv2.bias"), (1, 1))
