"""CPU-side checks of the C-ABI library: it loads, exports every symbol that
include/gf_hip.h declares, and validates arguments before touching a device."""
import ctypes
import os
import re

from gaussianformer_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared():
    text = open(os.path.join(ROOT, "include", "gf_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(gf_[a-z_0-9]+)\s*\(", text)))


def test_library_exports_every_declared_symbol():
    lib = _lib.load()
    names = _declared()
    assert len(names) >= 9
    for n in names:
        assert hasattr(lib, n), f"libgf_hip.so does not export {n}"
        assert n in _lib.SIGNATURES, f"_lib.SIGNATURES lacks {n}"
    assert sorted(_lib.SIGNATURES) == names


def test_version_and_sizes():
    lib = _lib.load()
    assert lib.gf_abi_version() == _lib.GF_ABI_VERSION
    assert lib.gf_splat_state_bytes() >= 64
    small = lib.gf_splat_workspace_bytes(100, 1000, 20, 20, 16)
    big = lib.gf_splat_workspace_bytes(25601, 640000, 200, 200, 16)
    assert 0 < small < big < (1 << 30)
    assert lib.gf_splat_workspace_bytes(-1, 0, 20, 20, 16) == 0


def test_argument_validation_without_gpu():
    lib = _lib.load()
    # 17 channels -> GF_EINVAL before any HIP call
    rc = lib.gf_splat_forward(0, 0, 0, 1, 1, 17, 8, 8, 8, *([None] * 13), None, 0, None)
    assert rc == -1 and b"18" in lib.gf_last_error()
    rc = lib.gf_splat_forward(7, 0, 0, 1, 1, 18, 8, 8, 8, *([None] * 13), None, 0, None)
    assert rc == -1 and b"variant" in lib.gf_last_error()
    rc = lib.gf_splat_forward(0, 0, 0, 1, 1, 18, 4096, 8, 8, *([None] * 13), None, 0, None)
    assert rc == -1
    rc = lib.gf_daf_forward(1, 6, 100, 128, 4, 10, 5, *([None] * 7))
    assert rc == -1 and b"divisible" in lib.gf_last_error()


def test_ops_fail_loudly_on_cpu_tensors():
    import pytest
    import torch
    import local_aggregate
    agg = local_aggregate.LocalAggregator(3, 8, 8, 8, [-2.0, -2.0, -2.0], 0.5)
    z = torch.zeros
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        agg(z(1, 4, 3), z(1, 2, 3), z(1, 2), z(1, 2, 18), z(1, 2, 3) + 0.2, torch.eye(3).repeat(1, 2, 1, 1))
    from model.encoder.gaussian_encoder.ops import DeformableAggregationFunction as DAF
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        DAF.apply(z(1, 1, 4, 8), torch.tensor([[2, 2]]), torch.tensor([0]), z(1, 3, 1, 2), z(1, 3, 1, 1, 4))


def test_ctypes_signatures_match_the_header_prototypes():
    """Argument count and class (pointer / integer / long long / size_t / float) of every prototype in
    include/gf_hip.h against gaussianformer_amd._lib.SIGNATURES -- a mismatch would not fail at load time, it
    would pass garbage."""
    import ctypes
    import os
    import re
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "gf_hip.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    protos = re.findall(r"\b(?:int|size_t|void|const char \*)\s*\*?\s*(gf_\w+)\s*\(([^;{]*?)\)\s*;", header, flags=re.S)
    assert len(protos) == len(_lib.SIGNATURES)

    def klass(decl):
        decl = " ".join(decl.split())
        if decl == "void":
            return None
        if "*" in decl:
            return "ptr"
        if decl.startswith("long long"):
            return "ll"
        if decl.startswith("size_t"):
            return "size"
        if decl.startswith("float"):
            return "float"
        assert decl.startswith("int"), decl
        return "int"

    def klass_c(t):
        if t in (ctypes.c_void_p, ctypes.c_char_p) or (isinstance(t, type) and issubclass(t, ctypes._Pointer)):
            return "ptr"
        return {ctypes.c_longlong: "ll", ctypes.c_size_t: "size", ctypes.c_float: "float", ctypes.c_int: "int"}[t]

    for name, args in protos:
        want = [k for k in (klass(a) for a in args.split(",")) if k]
        restype, argtypes = _lib.SIGNATURES[name]
        got = [klass_c(t) for t in argtypes]
        assert got == want, (name, got, want)


def test_python_constants_match_the_header_defines():
    """Every GF_* constant gaussianformer_amd._lib mirrors has the value include/gf_hip.h gives it (flags, path and
    verdict codes, the ABI version): a drifted flag would silently select another kernel."""
    text = open(os.path.join(ROOT, "include", "gf_hip.h")).read()
    defines = {m.group(1): int(m.group(2), 0) for m in re.finditer(r"^#define\s+(GF_[A-Z0-9_]+)\s+(-?(?:0x[0-9a-fA-F]+|\d+))\b", text, flags=re.M)}
    assert defines["GF_ABI_VERSION"] == _lib.GF_ABI_VERSION
    mirrored = [n for n in dir(_lib) if n.startswith("GF_") and isinstance(getattr(_lib, n), int)]
    assert len(mirrored) >= 15
    protocol = ("GF_STATE_NOT_DENSE GF_STATE_PATH GF_STATE_VERDICT GF_STATE_GENERATION GF_STATE_ROWS GF_STATE_WORDS GF_VERDICT_POINT "
                "GF_VERDICT_LATTICE GF_VERDICT_THETA GF_VERDICT_OPASEM GF_ROWS_READY GF_ROWS_OVERFLOW GF_SPLAT_FLAG_BYTES").split()
    assert set(protocol) <= set(mirrored)   # the state block's words and bits, the flag section's size
    for n in mirrored:
        assert n in defines, f"{n} is not defined in include/gf_hip.h"
        assert defines[n] == getattr(_lib, n), (n, defines[n], getattr(_lib, n))


def _streamed():
    """The entry points that launch: their last parameter is ``void *stream`` (include/gf_hip.h)."""
    text = open(os.path.join(ROOT, "include", "gf_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    protos = re.findall(r"\b(gf_\w+)\s*\(([^;{]*?)\)\s*;", text, flags=re.S)
    names = sorted(n for n, args in protos if re.search(r"\bvoid\s*\*\s*stream\s*$", args))
    assert len(names) >= 30 and all(_lib.SIGNATURES[n][1][-1] is ctypes.c_void_p for n in names)
    return names


def test_every_launch_goes_through_the_helper():
    """No module of the package enters a device guard or calls a launching entry point itself: ``_lib.call`` does both, so
    the guard, the stream and the name in the error cannot be forgotten or mistyped per op.  The one exception is
    ``SplatForwardPlan.run`` (gaussianformer_amd/local_aggregate.py), the pre-bound call the benchmark times."""
    import glob
    direct = re.compile(r"\.\s*(" + "|".join(_streamed()) + r")\s*\(")
    paths = sorted(glob.glob(os.path.join(ROOT, "gaussianformer_amd", "*.py")))
    assert len(paths) >= 15
    for path in paths:
        if os.path.basename(path) == "_lib.py":
            continue
        src = open(path).read()
        if os.path.basename(path) == "local_aggregate.py":
            run = re.search(r"\n    def run\(self, stream=None\):\n.*?\n(?=    def )", src, flags=re.S)
            assert run is not None and src.index("class SplatForwardPlan:") < run.start() < src.index("class SplatForwardPipeline:")
            assert "self.lib.gf_splat_forward(*self.args, stream)" in run.group(0)
            src = src[:run.start()] + src[run.end():]
        assert "torch.cuda.device(" not in src, path
        assert direct.search(src) is None, (path, direct.search(src).group(0))


def test_call_marshals_and_names_the_entry_point():
    """``_lib.call`` through the argument validation of ``gf_splat_forward`` (17 channels, as
    test_argument_validation_without_gpu): the error carries the entry point's name and the library's message.  There is no
    GPU here and ``torch.cuda.device`` cannot be entered for a CPU device, so ``call`` gives a device that is not a GPU no
    guard and a NULL stream -- the library refuses these arguments before any HIP call."""
    import pytest
    import torch
    cpu = torch.device("cpu")
    with pytest.raises(RuntimeError, match=r"gf_splat_forward failed \(code -1\): .*18"):
        _lib.call("gf_splat_forward", cpu, 0, 0, 0, 1, 1, 17, 8, 8, 8, *([None] * 13), None, 0)
    with pytest.raises(RuntimeError, match=r"gf_daf_forward_pinned failed .*divisible"):
        _lib.call("gf_daf_forward_pinned", cpu, 1, 6, 100, 128, 4, 10, 5, *([None] * 6))
    with pytest.raises(AttributeError):
        _lib.call("gf_no_such_entry_point", cpu)
    # tensors cross as their data pointers (the library sees a non-NULL pts and still refuses the channel count)
    t = torch.zeros(4)
    with pytest.raises(RuntimeError, match="gf_splat_forward failed"):
        _lib.call("gf_splat_forward", cpu, 0, 0, 0, 1, 1, 17, 8, 8, 8, t, *([None] * 12), None, 0)


def test_as_arg():
    import torch
    assert _lib.as_arg(None) is None
    x = torch.arange(12.0).reshape(3, 4).requires_grad_(True)
    a = _lib.as_arg(x)
    assert not a.requires_grad and a.data_ptr() == x.data_ptr()          # detached, no copy when nothing is to do
    b = _lib.as_arg(x.t(), torch.int32)
    assert b.dtype == torch.int32 and b.is_contiguous() and b.tolist() == x.t().int().tolist()
    m = torch.ones(5, dtype=torch.bool)
    assert _lib.as_arg(m, torch.bool).data_ptr() == m.data_ptr()


def test_stream_scratch():
    """The per-(device, stream) scratch cache, on CPU tensors with a stand-in for the current stream."""
    import torch
    cpu = torch.device("cpu")
    stream = [0]
    splat = _lib.StreamScratch(min_bytes=1 << 20, zeroed_bytes=_lib.GF_SPLAT_FLAG_BYTES, stream_of=lambda device: stream[0])
    other = _lib.StreamScratch(stream_of=lambda device: stream[0])
    a = splat.get(cpu, 100)
    assert a.dtype == torch.uint8 and a.numel() == 1 << 20 and not a[:_lib.GF_SPLAT_FLAG_BYTES].any()     # minimum size, zeroed flag section
    a[:_lib.GF_SPLAT_FLAG_BYTES] = 7
    assert splat.get(cpu, 4096).data_ptr() == a.data_ptr() and bool((a[:_lib.GF_SPLAT_FLAG_BYTES] == 7).all())   # reused, never zeroed again
    big = splat.get(cpu, (1 << 20) + 1)
    assert big.numel() == (1 << 20) + 1 and not big[:_lib.GF_SPLAT_FLAG_BYTES].any()                       # grows ...
    assert splat.get(cpu, 100).data_ptr() == big.data_ptr()                             # ... and never shrinks
    assert other.get(cpu, 100).numel() == 100                                           # no minimum of its own
    # stamp(): moved by any hand-out of the same cache, not by another cache's
    s0 = splat.stamp(cpu)
    assert s0 == splat.stamp(cpu) and s0[1] == big.data_ptr()
    other.get(cpu, 100)
    assert splat.stamp(cpu) == s0
    splat.get(cpu, 100)
    assert splat.stamp(cpu) != s0
    # at most MAX_STREAMS buffers, the most recently used ones
    assert _lib.StreamScratch.MAX_STREAMS == 8
    for s in range(1, 8):
        stream[0] = s
        splat.get(cpu, 100)
    assert len(splat._cache) == 8
    stream[0] = 0
    assert splat.get(cpu, 100).data_ptr() == big.data_ptr()      # stream 0 is the most recently used now
    stream[0] = 8
    splat.get(cpu, 100)                                          # a ninth stream: the least recently used (1) goes
    assert len(splat._cache) == 8
    kept = sorted(k[2] for k in splat._cache)
    assert kept == [0, 2, 3, 4, 5, 6, 7, 8]
    stream[0] = 0
    assert splat.get(cpu, 100).data_ptr() == big.data_ptr()
