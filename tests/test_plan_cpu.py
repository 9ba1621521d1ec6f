"""The host-only parts of the static executor (mis_hip.plan / mis_hip.swin_plan): the declared per-pass context and the one
import cycle between the two modules."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "cv-ssl-mis_amd")

# what an op sees on a context no plan has touched: no side stream, nothing queued, no pre-split weights, a differentiable pass
OFF = {"no_backward": False, "b3_fwd": False, "b3_bwd": False, "wgrad_stream": None, "deferred": None, "finals": None,
       "finals_bytes": 0, "final_batches": None}


def test_ctx_declares_every_field_off():
    from mis_hip.plan import Ctx
    ctx = Ctx(True)
    assert set(Ctx.__slots__) == set(OFF) | {"training", "rng_stream", "dropout", "state", "drop_masks"}
    assert not hasattr(ctx, "__dict__")
    for name, off in OFF.items():
        v = getattr(ctx, name)
        assert type(v) is type(off) and v == off, (name, v)
    assert (ctx.training, ctx.state, ctx.drop_masks, ctx.dropout, ctx.rng_stream) == (True, None, None, True, 0)
    state = object()
    ctx = Ctx(False, state=state, rng_stream=2)
    assert (ctx.training, ctx.state, ctx.rng_stream) == (False, state, 2)


def test_ctx_refuses_an_unknown_field():
    from mis_hip.plan import Ctx
    ctx = Ctx(True)
    with pytest.raises(AttributeError):
        ctx.wgrad_strem = None          # a misspelt field must not silently select the one-stream path
    with pytest.raises(AttributeError):
        ctx.no_backwards


@pytest.mark.parametrize("first, second", [("mis_hip.swin_plan", "mis_hip.plan"), ("mis_hip.plan", "mis_hip.swin_plan")])
def test_either_module_imports_first(first, second):
    code = (f"import sys; sys.path.insert(0, {PKG!r}); import {first}; import {second}; "
            "from mis_hip import plan, swin_plan; "
            "assert swin_plan.TAct is plan.TAct and issubclass(swin_plan.SwinPlan, plan.PlanBase) "
            "and issubclass(plan.Plan, plan.PlanBase) and not issubclass(plan.TAct, plan.Act); print('ok')")
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stderr
