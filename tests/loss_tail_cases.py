"""What the loss-tail GPU tests share (tests/test_loss_tails_gpu.py, tests/test_triple_tail_gpu.py): the rule's K, the weight,
the spatial shapes by name, the padding of a strided batch row, planted arg-max ties and the device step state."""
import torch

K = 6.0
W = 0.37
MAX_IT = 1000
PAD = 8          # batch stride C*S + 4*k, k = 2
SHAPES = {"2d": (1, 32, 48), "3d": (8, 12, 16), "part": (1, 40, 52), "odd": (1, 7, 9), "sq": (1, 36, 36),
          "bigvec": (140, 140, 143), "bigscalar": (11, 151, 421)}


def plant_ties(o, C):
    """Arg-max ties over three quarters of the voxels of ``o`` [n, C, ...]: all classes equal; the two largest equal at
    positions (0, 2) ((0, 1) for C == 2); -0.0 at class 0 against +0.0 at class 1, the rest negative."""
    flat = o.reshape(o.shape[0], C, -1)
    S = flat.shape[2]
    idx = torch.arange(S)
    flat[:, :, idx[idx % 4 == 0]] = 1.5
    second = 2 if C > 2 else 1
    sel = idx[idx % 4 == 1]
    flat[:, :, sel] = flat[:, :, sel].clamp(max=2.0)
    flat[:, 0, sel] = 7.25
    flat[:, second, sel] = 7.25
    sel = idx[idx % 4 == 2]
    flat[:, :, sel] = -1.0
    flat[:, 0, sel] = -0.0
    flat[:, 1, sel] = 0.0
    return flat.reshape(o.shape)


def state(c, gate_on):
    from mis_hip import ops
    st = ops.new_step_state()
    # rampup 0: cons_weight = (float)consistency, the same fp32 value as the float argument
    ops.step_init(st, 1, c["it"], 0.01, MAX_IT, 0.99, W, 0.0, 150, 0 if gate_on else c["it"] + 1000)
    s = ops.read_step_state(st)
    assert s["cons_gate"] == (1.0 if gate_on else 0.0) and s["iter_num"] == c["it"]
    return st
