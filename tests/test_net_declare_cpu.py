"""What every HIP network declares -- names, kinds, shapes, dtypes, the initial values and their order of drawing from
torch's global CPU generator -- pinned against tests/golden/net_declarations.json, and ``spec()`` of the four networks that
have one against the constructor.  No GPU: ``HipNet._materialize`` is stubbed out, so a constructor stops after its
declarations and ``net._specs`` still holds the init tensors.

The fixture is this file's own output (``python tests/test_net_declare_cpu.py --write``) at the commit before the typed
declaration calls (HipNet._conv / _norm / _linear) replaced the per-network init helpers; ``--sha256`` prints one digest per
configuration over the raw bytes of every declared tensor, for an exact comparison of two commits on one machine.

Comparison rule.  Integer tensors and float tensors that are all 0 or all 1 compare exactly.  Drawn tensors compare at a
relative 1e-6 on sum(x^2) and on eight elements at fixed flat positions, and at 1e-6 * sqrt(N * sum(x^2)) on sum(x): two
machines may round a vectorised erfinv / log differently by an ulp (6e-8), 1e-6 leaves a factor of sixteen over that, while a
changed law, order or shape moves every sampled element by its own magnitude.
"""
import hashlib
import json
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "cv-ssl-mis_amd")
for p in (PKG, ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

FIXTURE = os.path.join(ROOT, "tests", "golden", "net_declarations.json")
SEED = 20261020
RTOL = 1e-6


def _configs():
    from config import lite_config
    from networks.attention_unet import Attention_UNet
    from networks.discriminator import FC3DDiscriminator
    from networks.pnet import PNet2D
    from networks.projector import classifier, projectors
    from networks.swinunetr import SwinUNETR
    from networks.unet import UNet
    from networks.unet_3D import unet_3D
    from networks.unetr import UNETR
    from networks.vision_transformer import SwinUnet
    from networks.vnet import VNet
    # name -> (constructor, spec() with the matching arguments or None)
    cfg = {
        "unet": (lambda: UNet(1, 4), None),
        "unet_convtranspose": (lambda: UNet(1, 4, bilinear=False), None),
        "unet_3D": (lambda: unet_3D(n_classes=2, in_channels=1), None),
    }
    for n in ("batchnorm", "groupnorm", "instancenorm", "none"):
        cfg[f"vnet_{n}"] = (lambda n=n: VNet(1, 2, 16, n), None)
    cfg.update({
        "unetr": (lambda: UNETR(1, 2, (96, 96, 96)), None),
        "swinunetr": (lambda: SwinUNETR((96, 96, 96), 1, 2, feature_size=48), None),
        "swinunet": (lambda: SwinUnet(lite_config(), img_size=224, num_classes=4), None),
        "pnet": (lambda: PNet2D(1, 4, 64, [1, 2, 4, 8, 16]), lambda: PNet2D.spec(1, 4, 64, [1, 2, 4, 8, 16])),
        "attention_unet": (lambda: Attention_UNet(n_classes=2, in_channels=1),
                           lambda: Attention_UNet.spec(n_classes=2, in_channels=1)),
        "projectors": (lambda: projectors(), lambda: projectors.spec()),
        "classifier": (lambda: classifier(), lambda: classifier.spec()),
        "discriminator": (lambda: FC3DDiscriminator(2), lambda: FC3DDiscriminator.spec(2)),
    })
    return cfg


NAMES = ["unet", "unet_convtranspose", "unet_3D", "vnet_batchnorm", "vnet_groupnorm", "vnet_instancenorm", "vnet_none", "unetr",
         "swinunetr", "swinunet", "pnet", "attention_unet", "projectors", "classifier", "discriminator"]
WITH_SPEC = ["pnet", "attention_unet", "projectors", "classifier", "discriminator"]


def _build(name, patch):
    from mis_hip.plan import HipNet
    patch.setattr(HipNet, "_materialize", lambda self: None)
    torch.manual_seed(SEED)
    return _configs()[name][0]()


def _positions(n):
    return [k * (n - 1) // 7 for k in range(8)]


def _record_tensor(name, shape, kind, t):
    """[name, shape, value] (+ [kind, dtype] unless a float32 parameter).  value: 0 or 1 for a tensor that is all zeros or all
    ones, else [sum(x^2), sum(x), the eight elements] -- integers exactly, floats to 9 digits (a float32 element round-trips)."""
    assert tuple(t.shape) == tuple(shape), name
    flat = t.reshape(-1)
    at = _positions(flat.numel())
    const = next((c for c in (0, 1) if bool((flat == c).all())), None)
    if const is not None:
        value = const
    elif t.dtype.is_floating_point:
        d = flat.double()
        value = [float("%.9g" % v) for v in (float((d * d).sum()), float(d.sum()), *(float(d[i]) for i in at))]
    else:
        d = flat.long()
        value = [int((d * d).sum()), int(d.sum()), *(int(d[i]) for i in at)]
    rec = [name, list(shape), value]
    dtype = str(t.dtype).replace("torch.", "")
    return rec if (kind, dtype) == ("param", "float32") else rec + [kind, dtype]


def _record(name, net):
    rec = {"tensors": [_record_tensor(*s) for s in net._specs],
           "transposed_convs": sorted(getattr(net, "transposed_convs", ()))}
    spec = _configs()[name][1]
    if spec is not None:
        rec["spec"] = [[n, list(s)] for n, s in spec()]
    return rec


def _close(a, b, rel):
    return abs(a - b) <= rel * abs(b)


@pytest.fixture(scope="module")
def golden():
    with open(FIXTURE) as f:
        return json.load(f)


@pytest.mark.parametrize("name", NAMES)
def test_declarations_match_the_fixture(name, golden, monkeypatch):
    got, want = _record(name, _build(name, monkeypatch)), golden[name]
    assert got["transposed_convs"] == want["transposed_convs"]
    assert got.get("spec") == want.get("spec")
    assert [t[0] for t in got["tensors"]] == [t[0] for t in want["tensors"]]
    for g, w in zip(got["tensors"], want["tensors"]):
        label = f"{name}: {w[0]}"
        assert g[1] == w[1] and g[3:] == w[3:], (label, g, w)            # shape; kind and dtype
        gv, wv = g[2], w[2]
        if not isinstance(wv, list) or "int" in (w[4] if len(w) > 3 else ""):      # all zeros, all ones, integers: exactly
            assert gv == wv, (label, gv, wv)
            continue
        assert isinstance(gv, list), (label, gv, wv)
        n = 1
        for s in w[1]:
            n *= s
        assert _close(gv[0], wv[0], RTOL), (label, gv[0], wv[0])
        assert abs(gv[1] - wv[1]) <= RTOL * (n * wv[0]) ** 0.5, (label, gv[1], wv[1])
        assert all(_close(a, b, RTOL) for a, b in zip(gv[2:], wv[2:])), (label, gv[2:], wv[2:])


@pytest.mark.parametrize("name", WITH_SPEC)
def test_spec_draws_nothing_and_is_what_the_constructor_declares(name, monkeypatch):
    spec = _configs()[name][1]
    torch.manual_seed(SEED)
    before = torch.random.get_rng_state()
    listed = spec()
    assert torch.equal(torch.random.get_rng_state(), before), "spec() drew from the global generator"
    net = _build(name, monkeypatch)
    assert listed == [(n, s) for n, s, _, _ in net._specs]
    assert all(type(s) is tuple and all(type(v) is int for v in s) for _, s in listed)


def _sha256(name, net):
    h = hashlib.sha256()
    for n, shape, kind, t in net._specs:
        h.update(f"{n}|{kind}|{tuple(shape)}|{t.dtype}|".encode())
        h.update(t.contiguous().numpy().tobytes())
    h.update(repr(sorted(getattr(net, "transposed_convs", ()))).encode())
    return h.hexdigest()


if __name__ == "__main__":
    mode = sys.argv[1] if len(sys.argv) > 1 else ""
    if mode not in ("--write", "--sha256"):
        sys.exit("usage: test_net_declare_cpu.py --write | --sha256")
    out = {}
    with pytest.MonkeyPatch.context() as mp:
        for name in NAMES:
            net = _build(name, mp)
            if mode == "--sha256":
                print(f"{name:20s} {_sha256(name, net)}")
            else:
                out[name] = _record(name, net)
    if mode == "--write":
        with open(FIXTURE, "w") as f:       # one line per tensor: a changed entry shows as one changed line
            f.write("{\n")
            dumps = lambda v: json.dumps(v, separators=(",", ":"))
            for i, (name, rec) in enumerate(out.items()):
                f.write(f' "{name}": {{\n  "transposed_convs": {dumps(rec["transposed_convs"])},\n')
                if "spec" in rec:
                    f.write(f'  "spec": {dumps(rec["spec"])},\n')
                f.write('  "tensors": [\n' + ",\n".join(dumps(t) for t in rec["tensors"]) + "\n  ]\n }")
                f.write(",\n" if i + 1 < len(out) else "\n")
            f.write("}\n")
