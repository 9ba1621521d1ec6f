"""The declarations (HipNet._conv / _norm / _linear) on the device: a network built on the GPU holds, bit for bit, the tensors
the same seed declares on the host, in ``spec()``'s order, each parameter on a 16-byte boundary of ``flat_param`` with zero
padding words.  The smallest networks: ``classifier`` (convolutions, BatchNorm) and a narrow ``PNet2D``, the latter once
more with odd widths.  Nothing is launched: the networks are built, not run."""
import pytest
import torch

pytestmark = pytest.mark.gpu

SEED = 20261020


def _cases():
    from networks.pnet import PNet2D
    from networks.projector import classifier
    return {"classifier": (lambda: classifier(), lambda: classifier.spec()),
            "pnet": (lambda: PNet2D(1, 4, 8, [1, 2, 4, 8, 16]), lambda: PNet2D.spec(1, 4, 8, [1, 2, 4, 8, 16])),
            # every size of the two above is a multiple of 4 floats: odd widths for parameters that do end in padding
            "pnet_odd": (lambda: PNet2D(1, 3, 7, [1, 2, 4, 8, 16]), lambda: PNet2D.spec(1, 3, 7, [1, 2, 4, 8, 16]))}


@pytest.mark.parametrize("name", ["classifier", "pnet", "pnet_odd"])
def test_device_net_holds_the_host_declarations(name):
    from mis_hip.plan import HipNet
    make, spec = _cases()[name]
    with pytest.MonkeyPatch.context() as mp:        # the host side: a constructor that stops after its declarations
        mp.setattr(HipNet, "_materialize", lambda self: None)
        torch.manual_seed(SEED)
        host = {n: (kind, t) for n, _, kind, t in make()._specs}
    torch.manual_seed(SEED)
    net = make()
    sd = net.state_dict()
    assert list(sd) == [n for n, _ in spec()] == list(host)
    for n, (kind, t) in host.items():
        assert sd[n].dtype == t.dtype and tuple(sd[n].shape) == tuple(t.shape), n
        assert torch.equal(sd[n].cpu(), t), n
    params = [n for n, (kind, _) in host.items() if kind == "param"]
    assert list(net._offsets) == params == [n for n, _ in net.named_parameters()]
    used = torch.zeros(net.flat_param.numel(), dtype=torch.bool)
    end = 0
    for n in params:
        off, numel, shape = net._offsets[n]
        assert off % 4 == 0 and off == (end + 3) // 4 * 4, n
        assert sd[n].data_ptr() == net.flat_param.data_ptr() + 4 * off, n
        used[off:off + numel] = True
        end = off + numel
    assert net.flat_param.numel() == (end + 3) // 4 * 4
    assert bool((~used).any()) == (name == "pnet_odd")
    assert not net.flat_param.cpu()[~used].any() and not net.flat_grad.cpu().any()
