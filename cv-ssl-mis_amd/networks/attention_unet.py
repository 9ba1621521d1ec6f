"""Attention U-Net (``--model attention_unet``) on hand-written gfx950 kernels.

Drop-in for the reference's ``networks.attention_unet.Attention_UNet`` (code/networks/attention_unet.py:9-103, with
``GridAttentionBlock3D`` of code/networks/grid_attention_layer.py:7-107 and ``UnetGridGatingSignal3`` / ``UnetDsv3`` of
code/networks/utils.py:192-212,455-462): same constructor arguments, ``forward(x[N,C,D,H,W]) -> logits[N,n_classes,D,H,W]``
(the reference discards the attention maps too) and the same 141 state_dict entries in the same order -- ``conv{1-4}``,
``center``, ``gating.conv1.0.*``, ``attentionblock{2,3,4}.gate_block_{1,2}.{W.0, W.1, theta, phi, psi}.*``,
``attentionblock*.combine_gates.{0,1}.*``, ``up_concat{4-1}.conv.*``, ``dsv{4,3,2}.dsv.0.*``, ``dsv1.*``, ``final.*``.

Encoder and decoder are ``unet_3D``'s (UnetConv3 = (conv3x3x3 - InstanceNorm3d - ReLU) x 2, MaxPool3d(2), trilinear x2 +
concatenation) without its two dropouts, and take the same fusions.  On top of them, per level l in {2, 3, 4} with the skip
tensor x_l [C] and the gating signal g one level below (``gating(center)`` for level 4, the decoder output below otherwise):

    theta_k = Conv3d(C -> C, 2, stride 2, no bias)(x_l),  phi_k = Conv3d(Cg -> C, 1)(g)        k = 1, 2: two gates
    att_k   = sigmoid(psi_k(relu(theta_k + phi_k)))                    mis_attn_gate_map_*   (one [N, 2C] buffer each)
    y       = [up2(att_1) x_l, up2(att_2) x_l]                         mis_attn_gate_apply_*  (x_l read once)
    skip    = ReLU(BN(combine([BN(W_1 y_1), BN(W_2 y_2)])))            written into the decoder's concat buffer

``F.upsample(phi_g, size=theta_x.size()[2:])`` of the reference is an identity here -- the gating signal lives one level below
the skip and theta halves the skip -- and is not built; an input for which it would not be (D, H, W not multiples of 16) is
refused, as ``unet_3D`` refuses it.  The deep-supervision heads are 1x1x1 convolutions at their level followed by
trilinear up-sampling by 8 / 4 / 2 (mis_upsample_int_* / mis_upsample2_*) into channel slices of one [N, 4 n_classes] buffer
(``torch.cat`` never runs), ``final`` is a 1x1x1 convolution on that buffer.  Weights: ``init_weights(..., 'kaiming')``
(networks_other.py:40-49): kaiming_normal(fan_in) for every convolution, N(1, 0.02) / 0 for the BatchNorm affine parameters.

The layer graph is executed by ``mis_hip.plan``; nothing here computes on the CPU.
"""
from mis_hip.plan import HipNet


class Attention_UNet(HipNet):
    ndim_spatial = 3

    @classmethod
    def spec(cls, feature_scale=4, n_classes=21, in_channels=3):
        """[(state_dict key, shape)] in the reference's order."""
        return cls._declared(feature_scale, n_classes, in_channels)

    def _layers(self, feature_scale, n_classes, in_channels):
        """``init_weights(..., 'kaiming')``: kaiming_normal_ for every convolution (its bias keeps torch's default), N(1, 0.02)
        for the BatchNorm weights."""
        f = [int(x / feature_scale) for x in (64, 128, 256, 512, 1024)]

        def conv(prefix, cout, cin, k, bias=True):
            self._conv(prefix, cout, cin, k, bias, law="normal")

        def bn(prefix, C):
            self._norm(prefix, C, running=True, weight_std=0.02)

        def unetconv(prefix, cin, cout):
            conv(f"{prefix}.conv1.0", cout, cin, (3, 3, 3))
            conv(f"{prefix}.conv2.0", cout, cout, (3, 3, 3))

        cin = in_channels
        for n, co in zip(["conv1", "conv2", "conv3", "conv4", "center"], f):
            unetconv(n, cin, co)
            cin = co
        conv("gating.conv1.0", f[4], f[4], (1, 1, 1))
        for lvl in (2, 3, 4):
            C, Cg = f[lvl - 1], f[lvl]
            for k in (1, 2):
                p = f"attentionblock{lvl}.gate_block_{k}"
                conv(f"{p}.W.0", C, C, (1, 1, 1))
                bn(f"{p}.W.1", C)
                conv(f"{p}.theta", C, C, (2, 2, 2), bias="discard")     # bias-free, its bias draw is made and dropped
                conv(f"{p}.phi", C, Cg, (1, 1, 1))
                conv(f"{p}.psi", 1, C, (1, 1, 1))
            conv(f"attentionblock{lvl}.combine_gates.0", C, 2 * C, (1, 1, 1))
            bn(f"attentionblock{lvl}.combine_gates.1", C)
        for lvl in (4, 3, 2, 1):
            unetconv(f"up_concat{lvl}.conv", f[lvl] + f[lvl - 1], f[lvl - 1])
        for lvl in (4, 3, 2):
            conv(f"dsv{lvl}.dsv.0", n_classes, f[lvl - 1], (1, 1, 1))
        conv("dsv1", n_classes, f[0], (1, 1, 1))
        conv("final", n_classes, 4 * n_classes, (1, 1, 1))

    def __init__(self, feature_scale=4, n_classes=21, is_deconv=True, in_channels=3, nonlocal_mode='concatenation',
                 attention_dsample=(2, 2, 2), is_batchnorm=True):
        super().__init__()
        if not is_batchnorm or nonlocal_mode != 'concatenation' or tuple(attention_dsample) != (2, 2, 2):
            raise NotImplementedError("only is_batchnorm=True, nonlocal_mode='concatenation' and attention_dsample=(2,2,2) "
                                      "(the variant net_factory_3d builds) are on the HIP hot path")
        self.in_channels, self.n_classes = in_channels, n_classes
        self.filters = [int(x / feature_scale) for x in (64, 128, 256, 512, 1024)]
        self._layers(feature_scale, n_classes, in_channels)
        self._materialize()

    # UnetConv3 (networks/utils.py:99-123): (conv3x3x3 - InstanceNorm - ReLU) x 2
    def _unetconv(self, plan, prefix, x, cout, sp, out, need_dx=True):
        for sub, dst in (("conv1", None), ("conv2", out)):
            t = plan.new(cout, sp)
            plan.conv(x, t, self.P(f"{prefix}.{sub}.0.weight"), self.P(f"{prefix}.{sub}.0.bias"), (3, 3, 3),
                      need_dx=need_dx, bias_grad=False)
            y = dst if dst is not None else plan.new(cout, sp)
            plan.norm_act(t, y, per_sample=True, slope=0.0)
            x, need_dx = y, True
        return x

    def _bn(self, prefix, slope):
        P, B = self.P, self.B
        return dict(per_sample=False, gamma=P(f"{prefix}.weight"), beta=P(f"{prefix}.bias"),
                    running=(B(f"{prefix}.running_mean"), B(f"{prefix}.running_var"), B(f"{prefix}.num_batches_tracked")),
                    slope=slope)

    # MultiAttentionBlock (attention_unet.py:113-136) on the skip x [C, sp] and the gating signal g [Cg, sp / 2] -> out [C, sp]
    def _attention(self, plan, prefix, x, g, C, sp, sp2, out):
        P = self.P
        theta, phi = plan.new(2 * C, sp2), plan.new(2 * C, sp2)
        for k in (0, 1):
            p = f"{prefix}.gate_block_{k + 1}"
            plan.down_conv(x, plan.view(theta, k * C, C), P(f"{p}.theta.weight"), None)
            # phi's bias gradient is a channel sum of the buffer the gate map's backward writes: formed there (bias_grad=False)
            plan.conv(g, plan.view(phi, k * C, C), P(f"{p}.phi.weight"), P(f"{p}.phi.bias"), (1, 1, 1), bias_grad=False)
        att = plan.gate_map(theta, phi, plan.new(2, sp2),
                            [(P(f"{prefix}.gate_block_{k}.psi.weight"), P(f"{prefix}.gate_block_{k}.psi.bias")) for k in (1, 2)],
                            [P(f"{prefix}.gate_block_{k}.phi.bias") for k in (1, 2)])
        y = plan.gate_apply(x, att, plan.new(2 * C, sp))
        wy = plan.new(2 * C, sp)
        for k in (0, 1):
            p = f"{prefix}.gate_block_{k + 1}"
            t = plan.new(C, sp)
            # the bias in front of a BatchNorm has an exactly zero gradient (bias_grad=False)
            plan.conv(plan.view(y, k * C, C), t, P(f"{p}.W.0.weight"), P(f"{p}.W.0.bias"), (1, 1, 1), bias_grad=False)
            plan.norm_act(t, plan.view(wy, k * C, C), **self._bn(f"{p}.W.1", 1.0))        # BatchNorm3d, no activation
        t = plan.new(C, sp)
        plan.conv(wy, t, P(f"{prefix}.combine_gates.0.weight"), P(f"{prefix}.combine_gates.0.bias"), (1, 1, 1), bias_grad=False)
        return plan.norm_act(t, out, **self._bn(f"{prefix}.combine_gates.1", 0.0))

    def _build(self, plan):
        N, C, D, H, W = plan.in_shape
        if C != self.in_channels or D % 16 or H % 16 or W % 16:
            raise RuntimeError(f"Attention_UNet input must be [N,{self.in_channels},D,H,W] with D,H,W multiples of 16; "
                               f"got {plan.in_shape}")
        f, P, K = self.filters, self.P, self.n_classes
        sp = [(D >> l, H >> l, W >> l) for l in range(5)]
        cat = [plan.new(f[l] + f[l + 1], sp[l]) for l in range(4)]
        skip = [plan.view(cat[l], 0, f[l]) for l in range(4)]
        upv = [plan.view(cat[l], f[l], f[l + 1]) for l in range(4)]
        # encoder: conv1 goes straight into its decoder's concat buffer (no gate at level 1), conv2..4 are gated first
        enc = []
        x = plan.inp
        for l, name in enumerate(["conv1", "conv2", "conv3", "conv4"]):
            x = self._unetconv(plan, name, x, f[l], sp[l], skip[l] if l == 0 else plan.new(f[l], sp[l]), need_dx=(l > 0))
            enc.append(x)
            x = plan.maxpool(x, plan.new(f[l], sp[l + 1]))
        center = self._unetconv(plan, "center", x, f[4], sp[4], plan.new(f[4], sp[4]))
        t = plan.new(f[4], sp[4])
        plan.conv(center, t, P("gating.conv1.0.weight"), P("gating.conv1.0.bias"), (1, 1, 1), bias_grad=False)
        g = plan.norm_act(t, plan.new(f[4], sp[4]), per_sample=True, slope=0.0)
        # decoder (UnetUp3_CT, networks/utils.py:260-276; F.pad is a no-op for sizes divisible by 16) and the heads
        dsv = plan.new(4 * K, sp[0])
        x = center
        for lvl in (4, 3, 2, 1):
            l = lvl - 1
            if lvl > 1:
                self._attention(plan, f"attentionblock{lvl}", enc[l], g, f[l], sp[l], sp[l + 1], skip[l])
            plan.upsample(x, upv[l], align_corners=False)
            x = g = self._unetconv(plan, f"up_concat{lvl}.conv", cat[l], f[l], sp[l], plan.new(f[l], sp[l]))
            # UnetDsv3: 1x1x1 conv at this level, then trilinear x 2^l into its slice of [dsv1, dsv2, dsv3, dsv4]
            if lvl > 1:
                t = plan.new(K, sp[l])
                plan.conv(x, t, P(f"dsv{lvl}.dsv.0.weight"), P(f"dsv{lvl}.dsv.0.bias"), (1, 1, 1))
                plan.upsample(t, plan.view(dsv, l * K, K), align_corners=False, scale=1 << l)
            else:
                plan.conv(x, plan.view(dsv, 0, K), P("dsv1.weight"), P("dsv1.bias"), (1, 1, 1))
        plan.out = plan.new(K, sp[0])
        plan.conv(dsv, plan.out, P("final.weight"), P("final.bias"), (1, 1, 1))
