"""ctypes binding of the C-ABI HIP library (``libmis_hip.so``, declared in ``include/mis_hip.h``).

The product path has NO CPU fallback: if the shared library is missing or a
kernel entry point reports an error, a ``RuntimeError`` is raised.  torch is
only used for device memory (``tensor.data_ptr()``) and the current HIP stream.
"""
import ctypes
import os
import re

import torch  # imported first on purpose: libmis_hip.so binds to the libamdhip64 torch has loaded

_HERE = os.path.dirname(os.path.abspath(__file__))
# MIS_HIP_LIB overrides the library file (A/B timing of kernel variants); it is still a HIP build
LIB_PATH = os.environ.get("MIS_HIP_LIB") or os.path.join(_HERE, "libmis_hip.so")
HEADER_PATH = os.path.normpath(os.path.join(_HERE, "..", "..", "include", "mis_hip.h"))

_lib = None

_ERRORS = {
    -1: "MIS_ERR_ARG (bad pointer / size / stride)",
    -2: "MIS_ERR_UNSUPPORTED (shape not covered by the gfx950 kernel family)",
    -3: "MIS_ERR_LAUNCH (HIP launch failure)",
    -4: "MIS_ERR_WORKSPACE (workspace too small)",
}

_SCALARS = {"int": ctypes.c_int, "long long": ctypes.c_longlong, "float": ctypes.c_float, "double": ctypes.c_double,
            "unsigned": ctypes.c_uint, "unsigned int": ctypes.c_uint, "unsigned long long": ctypes.c_ulonglong}
_POINTEES = set(_SCALARS) | {"void", "char", "unsigned char", "MisStepState"}


def _ctype(text, decl):
    """The ctypes type of one return or parameter type as the header spells it; anything else is refused, never guessed."""
    t = " ".join(text.replace("*", " * ").split())
    if t in _SCALARS:
        return _SCALARS[t]
    if t == "char *":                          # the *_kernel_name out-buffers
        return ctypes.c_char_p
    m = re.fullmatch(r"(?:const )?([\w ]+) \*", t)
    if t == "mis_stream_t" or (m and m.group(1) in _POINTEES):
        return ctypes.c_void_p
    raise ValueError(f"mis_hip.h: {decl}: type {text.strip()!r} has no ctypes mapping")


def parse_header(text):
    """name -> (restype, argtypes) of every ``ret mis_name(type name, ...);`` in the text of a C header.  It understands what
    include/mis_hip.h holds and nothing more: comments, preprocessor lines, the extern "C" braces and typedefs are dropped,
    every statement left must be such a declaration with named parameters of the types _ctype knows."""
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)
    text = re.sub(r"^[ \t]*#.*$", " ", text, flags=re.M)
    text = re.sub(r'extern\s+"C"\s*\{|typedef\s+struct\s+\w+\s*\{[^{}]*\}\s*\w+\s*;|typedef\s[^;{}]*;', " ", text)
    *stmts, rest = text.split(";")
    if rest.strip() not in ("", "}"):
        raise ValueError(f"mis_hip.h: text after the last declaration: {rest.strip()!r}")
    protos = {}
    for stmt in stmts:
        stmt = " ".join(stmt.split())
        m = re.fullmatch(r"([\w ]+?) ?\b(mis_\w+) ?\(([^()]*)\)", stmt)
        if not m or m.group(2) in protos:
            raise ValueError(f"mis_hip.h: not a (single) function declaration: {stmt!r}")
        ret, name, args = m.groups()
        argtypes = []
        for arg in ([] if args.strip() == "void" else args.split(",")):
            p = re.fullmatch(r"(.*[\s*])(\w+)", arg.strip())       # type, parameter name
            if not p or p.group(2) in ("int", "long", "float", "double", "unsigned", "char", "void", "const"):
                raise ValueError(f"mis_hip.h: {name}: parameter {arg.strip()!r} is not `type name`")
            argtypes.append(_ctype(p.group(1), name))
        protos[name] = (_ctype(ret, name), argtypes)
    return protos


def _read_header(path=HEADER_PATH):
    if not os.path.exists(path):
        raise RuntimeError(f"{path} is missing: the ctypes prototypes are read from the C header of the checkout.")
    with open(path) as f:
        return parse_header(f.read())


# name -> (restype, argtypes), read from include/mis_hip.h -- the same text the library's definitions are compiled against
PROTOTYPES = _read_header()
# headers beside mis_hip.h that declare one kernel family each (same conventions, same parser): file name -> prototypes
EXTRA_HEADERS = ("mis_hip_fixmatch.h", "mis_hip_contrastive.h", "mis_hip_dilated.h", "mis_hip_attention_gate.h",
                 "mis_hip_adversarial.h", "mis_hip_adversarial2d.h")
EXTRA_PROTOTYPES = {h: _read_header(os.path.join(os.path.dirname(HEADER_PATH), h)) for h in EXTRA_HEADERS}

STEP_STATE_BYTES = 40  # sizeof(MisStepState): static_assert in csrc/common.h
AUG2D_BYTES = 88       # sizeof(MisAug2D): static_assert in csrc/augment.hip
CROP3D_BYTES = 48      # sizeof(MisCrop3D): static_assert in csrc/augment.hip
SURFACE_RECORD_WORDS = 12   # 8-byte fields of mis_surface_metrics' result record


class StreamPtr(ctypes.c_void_p):
    """The hipStream_t argument of a launching entry point (``stream_ptr()``): what marks a call as a launch for a LaunchTape."""


class LaunchTape:
    """One training step as a flat list of ``(callable, args)``: every C-ABI launch the eager step issued (the ctypes function and
    its already converted arguments: raw pointers into the plans' static buffers), the stream dependencies between them (HIP
    event record / wait pairs) and the Python callbacks of the gradient exchange (bucket all-reduces, on their streams).

    Why: the step is static -- same buffers, same launch sequence, the per-step scalars (RNG offset, learning rate, EMA alpha,
    consistency weight) live in a device-resident MisStepState -- but enqueueing it through the op graph costs the host 8 .. 10 ms
    of a 20 ms SwinUnet step (623 launches x ~14 us of Python per launch), and a captured hipGraph is no way out on this stack:
    replaying the SwinUnet step's graph costs the host 10.9 ms (measured, profiles/r06_*: ROCm enqueues the nodes one by one).
    Replaying the tape is one ctypes call per launch (~2.5 us).  ``recording()`` is the context the trainers run ONE eager step
    in; afterwards ``replay()`` is the step.  Everything the recorded step touched must stay where it is: inputs are copied
    into the static tensors the recording saw, grow-only scratch buffers are never freed (ops.scratch)."""

    def __init__(self):
        self.items = []
        self.keep = []          # objects the recorded arguments point into (events, tensors)

    def recording(self):
        return _Recording(self)

    def replay(self):
        for fn, args in self.items:
            st = fn(*args)
            if st:
                raise RuntimeError(f"launch tape: {getattr(fn, '__name__', fn)} failed with status {st}")

    def __len__(self):
        return len(self.items)


class _Recording:
    def __init__(self, tape):
        self.tape = tape

    def __enter__(self):
        global TAPE
        if TAPE is not None:
            raise RuntimeError("a launch tape is already being recorded")
        TAPE = self.tape
        return self.tape

    def __exit__(self, *exc):
        global TAPE
        TAPE = None
        return False


TAPE = None        # the LaunchTape being recorded (None: eager)


class _RecordingLib:
    """Stands in for the ctypes library while a tape is recorded: calls go through, launches (last argument a StreamPtr) are
    appended to the tape with their argument tuples."""

    def __init__(self, lib):
        self._lib = lib

    def __getattr__(self, name):
        fn = getattr(self._lib, name)

        def call(*args):
            st = fn(*args)
            # a refused call (MIS_ERR_UNSUPPORTED: the caller goes on to another entry point) launched nothing
            if st == 0 and TAPE is not None and args and isinstance(args[-1], StreamPtr):
                TAPE.items.append((fn, args))
            return st
        call.__name__ = name
        setattr(self, name, call)
        return call


_rec_lib = None


def load():
    """Load libmis_hip.so (once) and attach prototypes.  Raises if it is not built."""
    global _lib, _rec_lib
    if _lib is not None:
        if TAPE is not None:
            if _rec_lib is None:
                _rec_lib = _RecordingLib(_lib)
            return _rec_lib
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            f"{LIB_PATH} is missing: build it with `make -C cv-ssl-mis_amd/csrc` "
            "(or `python -c 'import __graft_entry__ as g; g.build()'`).  There is no CPU fallback.")
    lib = ctypes.CDLL(LIB_PATH)
    protos = dict(PROTOTYPES)
    for extra in EXTRA_PROTOTYPES.values():
        if set(extra) & set(protos):
            raise RuntimeError(f"declared twice: {sorted(set(extra) & set(protos))}")
        protos.update(extra)
    for name, (res, args) in protos.items():
        fn = getattr(lib, name)  # AttributeError if the .so does not export a declared symbol
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def check(status, what):
    if status != 0:
        raise RuntimeError(f"{what} failed: {_ERRORS.get(int(status), status)}")


def stream_ptr():
    """hipStream_t of torch's current stream, as a void*."""
    return StreamPtr(torch.cuda.current_stream().cuda_stream)


_hip = None


def _hip_runtime():
    """The libamdhip64 torch has loaded (for event record / wait pairs on a tape)."""
    global _hip
    if _hip is None:
        path = None
        with open("/proc/self/maps") as f:
            for line in f:
                if "libamdhip64.so" in line:
                    path = line.split()[-1]
                    break
        if path is None:
            raise RuntimeError("libamdhip64.so is not loaded in this process")
        h = ctypes.CDLL(path)
        h.hipEventCreateWithFlags.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_uint]
        h.hipEventRecord.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
        h.hipStreamWaitEvent.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint]
        for fn in (h.hipEventCreateWithFlags, h.hipEventRecord, h.hipStreamWaitEvent):
            fn.restype = ctypes.c_int
        _hip = h
    return _hip


def wait_stream(waiter, waited):
    """``waiter.wait_stream(waited)``; while a tape is recorded the dependency is an event record / wait pair of the tape's own
    (replayed as two HIP runtime calls)."""
    if TAPE is None:
        waiter.wait_stream(waited)
        return
    h = _hip_runtime()
    ev = ctypes.c_void_p()
    if h.hipEventCreateWithFlags(ctypes.byref(ev), 0x2) != 0:          # hipEventDisableTiming
        raise RuntimeError("hipEventCreateWithFlags failed")
    rec = (h.hipEventRecord, (ev, ctypes.c_void_p(waited.cuda_stream)))
    wai = (h.hipStreamWaitEvent, (ctypes.c_void_p(waiter.cuda_stream), ev, 0))
    for fn, args in (rec, wai):
        if fn(*args) != 0:
            raise RuntimeError("HIP event record / wait failed")
        TAPE.items.append((fn, args))
    TAPE.keep.append(ev)


def tape_call(fn, *args):
    """``fn(*args)`` now, and again -- with the stream that is current now -- at this point of every replay when a tape is being
    recorded (the Python side of the gradient exchange: torch.distributed collectives order themselves behind the current
    stream).  Returns fn's result."""
    r = fn(*args)
    if TAPE is not None:
        stream = torch.cuda.current_stream()

        def again():
            with torch.cuda.stream(stream):
                fn(*args)
        again.__name__ = getattr(fn, "__name__", "callback")
        TAPE.items.append((again, ()))
    return r


def ptr(t):
    """Raw device pointer of a tensor (None -> NULL)."""
    if t is None:
        return None
    return ctypes.c_void_p(t.data_ptr())


def _address(v):
    """A pointer argument that is neither None nor a plain torch.Tensor: a Parameter or another tensor subclass becomes its
    device address, anything else (an int address, a ctypes byref) is ctypes' to convert."""
    p = getattr(v, "data_ptr", None)
    return v if p is None else p()


_Tensor = torch.Tensor


def _operands(args):
    """The C arguments of a wrapper's operands: tuples -- (view, batch stride), (label, bytes per label), (workspace, bytes) --
    are flattened in order, a tensor becomes its device address and None stays NULL; ctypes converts the scalars itself.
    (On the host path of every eager launch: the common kinds are decided by their exact type, most frequent first.)"""
    out = []
    add = out.append
    for a in args:
        t = type(a)
        if t is _Tensor:
            add(a.data_ptr())
        elif t is int or t is float or a is None:
            add(a)
        elif t is tuple:
            for v in a:
                t = type(v)
                add(v.data_ptr() if t is _Tensor else v if (t is int or v is None) else _address(v))
        else:
            add(_address(a))
    return out


def launch(name, *args):
    """Launch the entry point ``name`` on torch's current stream; raises with that name on a non-zero status.  The function is
    looked up through load() on every call (a tape being recorded stands in for the library), and the stream is the last
    argument, a StreamPtr: what marks the call as a launch for the tape."""
    st = getattr(load(), name)(*_operands(args), stream_ptr())
    if st:
        check(st, name)


def try_launch(name, *args):
    """``launch`` for entry points that may refuse a shape: False on MIS_ERR_UNSUPPORTED (nothing was launched, nothing lands on
    a tape, the caller goes on to another entry point), True after a launch; every other status raises."""
    return _accepted(getattr(load(), name)(*_operands(args), stream_ptr()), name)


def supported(name, *args):
    """The same answer from an entry point without a stream that fills out-parameters for a shape or refuses it."""
    return _accepted(getattr(load(), name)(*_operands(args)), name)


def _accepted(st, name):
    if st == -2:
        return False
    if st:
        check(st, name)
    return True


def query(name, *args):
    """The int an entry point without a stream answers (sizes, counts, selectors); a negative answer is an error code and
    raises with that name."""
    n = getattr(load(), name)(*_operands(args))
    if n < 0:
        check(n, name)
    return n


def select(name, *args):
    """``query`` for the ``*_select`` entry points, whose negative answer is an answer ("no variant: use the direct kernel"),
    not an error: it is returned."""
    return int(getattr(load(), name)(*_operands(args)))


def kernel_name(name, *args):
    """What a ``*_kernel_name`` entry point prints for these arguments: the kernel a launch runs, as rocprofv3 names it."""
    buf = ctypes.create_string_buffer(128)
    query(name, *args, buf, 128)
    return buf.value.decode()


def require_gpu(*tensors):
    for t in tensors:
        if t is not None and not t.is_cuda:
            raise RuntimeError("mis_hip kernels need device tensors (HIP/gfx950); got a CPU tensor. "
                               "There is no CPU fallback in the product path.")
