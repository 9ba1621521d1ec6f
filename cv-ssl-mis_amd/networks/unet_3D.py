"""3-D U-Net (``--model unet_3D``) on hand-written gfx950 kernels.

Drop-in for the reference's ``networks.unet_3D.unet_3D`` (code/networks/unet_3D.py:20-94, built
from ``UnetConv3`` / ``UnetUp3_CT`` of code/networks/utils.py:99-123,260-276): same constructor
arguments, ``forward(x[N,1,D,H,W]) -> logits[N,n_classes,D,H,W]`` and state_dict keys
(``conv{1-4}.conv{1,2}.0.*``, ``center.conv{1,2}.0.*``, ``up_concat{4-1}.conv.conv{1,2}.0.*``, ``final.*``).

As instantiated by ``net_factory_3d`` (feature_scale=4, is_batchnorm=True): filters
[16,32,64,128,256]; every 3x3x3 conv is followed by InstanceNorm3d (no affine, no running stats)
and ReLU; MaxPool3d(2) between encoder levels; decoder = trilinear x2 (align_corners=False) ->
cat([skip, up]) -> UnetConv3; Dropout(0.3) after ``center`` and after ``up_concat1``; final 1x1x1
conv.  Weights: kaiming_normal(fan_in) like ``init_weights(..., 'kaiming')`` (networks_other.py:40-49).
"""
from mis_hip.plan import HipNet


class unet_3D(HipNet):
    ndim_spatial = 3

    def __init__(self, feature_scale=4, n_classes=21, is_deconv=True, in_channels=3, is_batchnorm=True):
        super().__init__()
        if not is_batchnorm:
            raise NotImplementedError("only the is_batchnorm=True variant (the one net_factory_3d builds) is on "
                                      "the HIP hot path")
        self.in_channels, self.n_classes = in_channels, n_classes
        self.filters = f = [int(x / feature_scale) for x in (64, 128, 256, 512, 1024)]
        names = ["conv1", "conv2", "conv3", "conv4", "center"]
        cin = in_channels
        for n, co in zip(names, f):
            self._declare_unetconv(n, cin, co)
            cin = co
        for lvl in (4, 3, 2, 1):
            self._declare_unetconv(f"up_concat{lvl}.conv", f[lvl] + f[lvl - 1], f[lvl - 1])
        self._conv("final", n_classes, f[0], (1, 1, 1), law="normal")
        self._materialize()

    def _declare_unetconv(self, prefix, cin, cout):
        self._conv(f"{prefix}.conv1.0", cout, cin, (3, 3, 3), law="normal")
        self._conv(f"{prefix}.conv2.0", cout, cout, (3, 3, 3), law="normal")

    # UnetConv3 (networks/utils.py:99-123): (conv3x3x3 - InstanceNorm - ReLU) x 2
    def _unetconv(self, plan, prefix, x, cout, sp, out, drop_p=0.0, need_dx=True):
        for sub, dst, p in (("conv1", None, 0.0), ("conv2", out, drop_p)):
            t = plan.new(cout, sp)
            plan.conv(x, t, self.P(f"{prefix}.{sub}.0.weight"), self.P(f"{prefix}.{sub}.0.bias"), (3, 3, 3),
                      need_dx=need_dx, bias_grad=False)
            y = dst if dst is not None else plan.new(cout, sp)
            plan.norm_act(t, y, per_sample=True, slope=0.0, drop_p=p)
            x, need_dx = y, True
        return x

    def _build(self, plan):
        N, C, D, H, W = plan.in_shape
        if C != self.in_channels or D % 16 or H % 16 or W % 16:
            raise RuntimeError(f"unet_3D input must be [N,{self.in_channels},D,H,W] with D,H,W multiples of 16; "
                               f"got {plan.in_shape}")
        f = self.filters
        sp = [(D >> l, H >> l, W >> l) for l in range(5)]
        cat = [plan.new(f[l] + f[l + 1], sp[l]) for l in range(4)]
        skip = [plan.view(cat[l], 0, f[l]) for l in range(4)]
        upv = [plan.view(cat[l], f[l], f[l + 1]) for l in range(4)]
        x = plan.inp
        for l, name in enumerate(["conv1", "conv2", "conv3", "conv4"]):
            x = self._unetconv(plan, name, x, f[l], sp[l], skip[l], need_dx=(l > 0))
            pooled = plan.new(f[l], sp[l + 1])
            plan.maxpool(x, pooled)
            x = pooled
        # center + dropout1 (unet_3D.py:84-85)
        x = self._unetconv(plan, "center", x, f[4], sp[4], plan.new(f[4], sp[4]), drop_p=0.3)
        # UnetUp3_CT (networks/utils.py:260-276); F.pad is a no-op for sizes divisible by 16
        for lvl in (4, 3, 2, 1):
            l = lvl - 1
            plan.upsample(x, upv[l], align_corners=False)
            x = self._unetconv(plan, f"up_concat{lvl}.conv", cat[l], f[l], sp[l], plan.new(f[l], sp[l]),
                               drop_p=0.3 if lvl == 1 else 0.0)   # dropout2 after up_concat1 (unet_3D.py:89-90)
        plan.out = plan.new(self.n_classes, sp[0])
        plan.conv(x, plan.out, self.P("final.weight"), self.P("final.bias"), (1, 1, 1), bias_grad=True)
