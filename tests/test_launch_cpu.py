"""The launch path of the C-ABI wrappers without a GPU (mis_hip/lib.py): how launch / try_launch / query marshal a wrapper's
operands, what they raise, and what of it lands on a LaunchTape."""
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "cv-ssl-mis_amd"))


class _FakeLib:
    """Entry points that log the arguments they were called with and answer ``status``."""

    def __init__(self):
        self.log = []
        self.status = 0

    def _entry(name):
        def call(self, *args):
            self.log.append((name, args))
            return self.status
        return call

    mis_launch = _entry("mis_launch")
    mis_other = _entry("mis_other")
    mis_size = _entry("mis_size")


@pytest.fixture
def fake(monkeypatch):
    from mis_hip import lib
    fake = _FakeLib()
    monkeypatch.setattr(lib, "_lib", fake)
    monkeypatch.setattr(lib, "_rec_lib", None)
    monkeypatch.setattr(lib, "stream_ptr", lambda: lib.StreamPtr(0x57))
    return fake


def test_launch_flattens_tuples_in_order_and_appends_the_stream(fake):
    from mis_hip import lib
    x, y = torch.zeros(4), torch.zeros(3, dtype=torch.uint8)
    lib.launch("mis_launch", x, 5, (y, 8), (None, 0), 2.5, (x, 1, 2), None)
    (name, args), = fake.log
    assert name == "mis_launch"
    assert list(args[:-1]) == [x.data_ptr(), 5, y.data_ptr(), 8, None, 0, 2.5, x.data_ptr(), 1, 2, None]
    assert type(args[-1]) is lib.StreamPtr and args[-1].value == 0x57


def test_tensor_subclasses_become_addresses_and_ctypes_arguments_pass_untouched(fake):
    import ctypes
    from mis_hip import lib
    p = torch.nn.Parameter(torch.zeros(4))          # not a plain torch.Tensor: the path beside the exact-type one
    n, buf = ctypes.c_int(0), ctypes.create_string_buffer(8)
    ref = ctypes.byref(n)
    lib.launch("mis_launch", p, (p, 4), ref, (None, ref), buf, 0x1000, True)
    args = fake.log[0][1]
    assert list(args[:3]) == [p.data_ptr(), p.data_ptr(), 4]
    assert args[3] is ref and args[4] is None and args[5] is ref and args[6] is buf      # ctypes converts these itself
    assert args[7] == 0x1000 and args[8] is True and type(args[9]) is lib.StreamPtr


def test_a_failed_launch_raises_with_the_called_name_and_the_error_text(fake):
    from mis_hip import lib
    for status, text in ((-1, "MIS_ERR_ARG"), (-3, "MIS_ERR_LAUNCH"), (-4, "MIS_ERR_WORKSPACE"), (-2, "MIS_ERR_UNSUPPORTED")):
        fake.status = status
        with pytest.raises(RuntimeError, match=f"mis_other failed: {text}"):
            lib.launch("mis_other", 1)


def test_try_launch_returns_false_on_unsupported_and_raises_on_anything_else(fake):
    from mis_hip import lib
    tape = lib.LaunchTape()
    with tape.recording():
        fake.status = -2
        assert lib.try_launch("mis_launch", 1) is False
        fake.status = -1
        with pytest.raises(RuntimeError, match="mis_launch failed: MIS_ERR_ARG"):
            lib.try_launch("mis_launch", 2)
        assert len(tape) == 0                         # neither the refused nor the failed call is a launch to replay
        fake.status = 0
        assert lib.try_launch("mis_launch", 3) is True
    assert [a[0] for _, a in tape.items] == [3]
    assert type(fake.log[0][1][-1]) is lib.StreamPtr  # the refusing variant passes the stream like launch does


def test_query_passes_sizes_through_and_raises_on_an_error_code(fake):
    from mis_hip import lib
    x = torch.zeros(2)
    for n in (0, 1, 1 << 40):
        fake.status = n
        assert lib.query("mis_size", (x, 3), None) == n
    assert fake.log[0] == ("mis_size", (x.data_ptr(), 3, None))          # marshalled like a launch, but no stream
    fake.status = -1
    with pytest.raises(RuntimeError, match="mis_size failed: MIS_ERR_ARG"):
        lib.query("mis_size", 1)
    fake.status = -2
    with pytest.raises(RuntimeError, match="mis_size failed: MIS_ERR_UNSUPPORTED"):
        lib.query("mis_size", 1)
    assert lib.select("mis_size", 1) == -2                              # a selector's negative answer is an answer
    assert lib.supported("mis_size", 1) is False
    fake.status = 0
    assert lib.supported("mis_size", 1) is True


def test_a_launch_made_while_a_tape_records_is_replayed_once_per_replay(fake):
    from mis_hip import lib
    x = torch.zeros(4)
    tape = lib.LaunchTape()
    lib.launch("mis_launch", x, 0)                    # before the recording: eager only
    with tape.recording():
        lib.launch("mis_launch", (x, 4), 1)
        assert lib.query("mis_size", 9) == 0          # no stream: not on the tape
        lib.launch("mis_other", None, 2)
    lib.launch("mis_launch", x, 3)                    # after it: the library itself again
    assert len(tape) == 2
    fake.log.clear()
    tape.replay()
    assert [(n, a[:-1]) for n, a in fake.log] == [("mis_launch", (x.data_ptr(), 4, 1)), ("mis_other", (None, 2))]
    assert all(type(a[-1]) is lib.StreamPtr for _, a in fake.log)
    tape.replay()
    assert len(fake.log) == 4
