"""CPU: the C-ABI library builds, loads and exports every symbol include/llark_hip.h declares
(no compute calls without a GPU)."""
import os
import re

from llark_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared_in_header():
    text = open(os.path.join(ROOT, "include", "llark_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(llark_[a-z0-9_]+)\s*\(", text)))


def test_header_symbols_exported():
    L = _lib.lib()
    names = _declared_in_header()
    assert len(names) >= 15
    for n in names:
        assert hasattr(L, n), f"{n} declared in include/llark_hip.h but not exported by libllark_hip.so"


def test_python_signatures_cover_header():
    assert _declared_in_header() == _lib.declared_symbols()


def test_header_parser_maps_every_type_and_refuses_to_guess():
    """_lib.parse_header on a literal header: every mapped type, const, a `[]` parameter, void / const char* / handle returns,
    comments and preprocessor lines; an unknown type or a prototype the pattern does not take raises instead of guessing."""
    import ctypes as C

    import pytest
    text = """
    #define LLARK_X 1
    typedef void* llark_stream_t; /* llark_not_a_function(int x); */
    typedef struct llark_workspace* llark_workspace_t;   // llark_nor_this(int y);
    int llark_a(const float* x, int n, int64_t big, long long bigger, unsigned u, const unsigned* up, float f,
                double d, char* name, const char *cname, void* p, const int idx[], uint8_t* bytes,
                llark_workspace_t ws, llark_stream_t stream);
    void llark_b(void* plan);
    const char* llark_c(void);
    llark_workspace_t llark_d(void);
    void* llark_e();
    long long llark_f(llark_stream_t stream, int after);
    """
    P, I = C.c_void_p, C.c_int
    got = _lib.parse_header(text)
    assert got == {
        "llark_a": (I, [P, I, C.c_int64, C.c_int64, C.c_uint, P, C.c_float, C.c_double, C.c_char_p, C.c_char_p, P, P, P, P, P], 14),
        "llark_b": (None, [P], None),
        "llark_c": (C.c_char_p, [], None),
        "llark_d": (P, [], None),
        "llark_e": (P, [], None),
        "llark_f": (C.c_int64, [P, I], 0),
    }
    with pytest.raises(_lib.LlarkHipError, match="size_t.*llark_g"):
        _lib.parse_header("int llark_g(size_t n);")
    with pytest.raises(_lib.LlarkHipError, match="short.*llark_g"):
        _lib.parse_header("short llark_g(int n);")
    with pytest.raises(_lib.LlarkHipError, match="llark_h"):                    # a callback parameter: not a plain prototype
        _lib.parse_header("int llark_g(int n);\nint llark_h(void (*cb)(int), int n);")


def test_python_signatures_are_the_headers():
    """What ctypes is told equals what the header declares, for every entry point; a stream is always the last parameter."""
    text = open(os.path.join(ROOT, "include", "llark_hip.h")).read()
    protos = _lib.parse_header(text)
    assert sorted(protos) == _declared_in_header() and len(protos) >= 118
    L = _lib.lib()
    for name, (restype, argtypes, stream) in protos.items():
        fn = getattr(L, name)
        assert list(fn.argtypes) == argtypes == _lib._SIGS[name] and fn.restype == restype, name
        assert stream == _lib._STREAM_ARG[name] and stream in (None, len(argtypes) - 1), name


def _llark_calls(tree):
    import ast
    for node in ast.walk(tree):
        if isinstance(node, ast.Call) and isinstance(node.func, ast.Attribute) and node.func.attr.startswith("llark_"):
            yield node


def test_every_call_site_passes_the_headers_argument_count():
    """Static: every `<expr>.llark_<name>(...)` under llark_amd/, tests/, scripts/ and in bench.py passes exactly the header's
    parameter count, positionally (calls with a starred argument cannot be counted and are skipped)."""
    import ast
    import pathlib
    root = pathlib.Path(ROOT)
    files = [root / "bench.py"] + [p for d in ("llark_amd", "tests", "scripts") for p in sorted((root / d).rglob("*.py"))]
    counted, bad = 0, []
    for path in files:
        for call in _llark_calls(ast.parse(path.read_text(), str(path))):
            if any(isinstance(a, ast.Starred) for a in call.args):
                continue
            counted += 1
            want = _lib._SIGS.get(call.func.attr)
            if want is None or len(call.args) != len(want) or call.keywords:
                bad.append(f"{path.relative_to(root)}:{call.lineno} {call.func.attr}: {len(call.args)} arguments, "
                           f"{len(call.keywords)} keywords, header declares {None if want is None else len(want)}")
    assert not bad, "\n".join(bad)
    assert counted >= 120, counted


def test_integration_md_argtypes_stubs_match_the_header():
    import ctypes
    env = {"ctypes": ctypes, "P": ctypes.c_void_p, "I": ctypes.c_int, "F": ctypes.c_float}     # as INTEGRATION.md binds them
    stubs = re.findall(r"^L\.(llark_\w+)\.argtypes = (.+)$", open(os.path.join(ROOT, "INTEGRATION.md")).read(), flags=re.M)
    assert len(stubs) >= 15
    for name, expr in stubs:
        assert eval(expr, env) == _lib._SIGS[name], name


def test_python_constants_equal_the_headers():
    from llark_amd import ops
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "llark_hip.h")).read(), flags=re.S)
    hdr = {k: int(v) for k, v in re.findall(r"\b(LLARK_[A-Z0-9_]+)\s*=\s*(-?\d+)", text)}
    hdr.update((k, int(v)) for k, v in re.findall(r"^#define\s+(LLARK_[A-Z0-9_]+)\s+(-?\d+)\s*$", text, flags=re.M))
    assert ops.F16 == hdr["LLARK_F16"] and ops.BF16 == hdr["LLARK_BF16"]
    for prefix in ("EPI_", "ROW_"):
        py = {k: getattr(ops, k) for k in dir(ops) if k.startswith(prefix)}
        assert py and py == {k[len("LLARK_"):]: v for k, v in hdr.items() if k.startswith("LLARK_" + prefix)}
    # the code ops.workspace() / ops.sk_scratch() hand to check() when a constructor fails
    import inspect
    for fn in (ops.workspace, ops.sk_scratch):
        assert re.findall(r"check\((-?\d+),", inspect.getsource(fn)) == [str(hdr["LLARK_ERR_LAUNCH"])]


def test_version_and_error_string():
    L = _lib.lib()
    assert L.llark_version() >= 100
    assert isinstance(L.llark_last_error(), bytes)


def test_invalid_arguments_are_reported_not_crashed():
    # argument validation happens before any HIP call, so this is safe without a GPU
    L = _lib.lib()
    rc = L.llark_gemm16(0, 1, 0, None, None, 0, None, 0, None, 0, 0, 0, None, 0, None, 0, None, None, 0, None)
    assert rc == -1
    assert b"gemm16" in L.llark_last_error()
    rc = L.llark_prior_attn(None, 0, 1, 64, 48, 2, 8, 1, None, None, 0, None)
    assert rc == -1
    # the decode and prefill attention entry points: the null check precedes any HIP call and names the entry point
    N = None
    for entry, says, args in [
        ("llark_attn_decode_bf16", "attn_decode", (N, N, N, N, N, N, 1, 2, 128, 8, 8, N, N, N)),
        ("llark_attn_decode_bf16_alibi", "attn_decode", (N, N, N, N, N, N, 1, 2, 128, 8, 8, N, N, N, N)),
        ("llark_attn_decode_bf16_dpos", "attn_decode_dpos", (N, N, N, N, N, N, 1, 2, 128, N, 8, N, N, N)),
        ("llark_attn_decode_rope_bf16", "attn_decode_rope", (N, 1, 2, 128, 0, N, N, N, 8, N, N, N, N, 8, N, N, N, N)),
        ("llark_attn_decode_rope_bf16_chain", "attn_decode_rope_chain", (N, 1, 2, 128, 0, N, N, N, 8, N, N, N, N, 8, N, N, N, N, N)),
        ("llark_attn_decode_rope_bf16_rows", "attn_decode_rope_rows", (N, 1, 2, 128, N, N, N, 8, N, N, N, N, 8, N, N, N, N)),
        ("llark_attn_prefill_bf16", "attn_prefill", (N, N, N, N, N, N, 1, 8, 2, 128, 0, 8, N, N, N)),
        ("llark_attn_prefill_bf16_alibi", "attn_prefill", (N, N, N, N, N, N, 1, 8, 2, 128, 0, 8, N, N, N, N)),
        ("llark_attn_prefill_bf16_lse", "attn_prefill_lse", (N, N, N, 1, 8, 2, 128, 8, N, N, N, N)),
    ]:
        assert getattr(L, entry)(*args) == -1, entry
        assert L.llark_last_error().startswith(says.encode() + b": null"), (entry, L.llark_last_error())


def test_product_package_never_imports_the_oracle():
    """The oracle is test infrastructure: nothing under llark_amd/ may import, call or link it (only tests/,
    __graft_entry__.smoke() and bench.py's cpu_baseline leg do)."""
    import pathlib
    import re
    root = pathlib.Path(__file__).resolve().parents[1] / "llark_amd"
    pat = re.compile(r"^\s*(from\s+oracle\b|import\s+oracle\b)|oracle/_build|libjukebox_ref", re.M)
    offenders = [str(p) for p in root.rglob("*.py") if pat.search(p.read_text())]
    inc = re.compile(r"#\s*include\s*[<\"][^>\"]*(oracle|jukebox_ref)[^>\"]*[>\"]")
    offenders += [str(p) for ext in ("*.hip", "*.h") for p in root.rglob(ext) if inc.search(p.read_text())]
    mk = root / "csrc" / "Makefile"
    assert "oracle" not in mk.read_text()
    assert not offenders, offenders


def test_launch_list_records_and_replays_c_abi_calls():
    """ops.LaunchList mechanics without a GPU: calls made through _lib.lib() while recording are kept in order with their
    arguments, replay re-issues them and surfaces a failing return code as LlarkHipError; recording does not nest."""
    import pytest
    from llark_amd import _lib as LB
    from llark_amd import ops as O
    O._stream = lambda: 0                                     # no device here; restored below
    try:
        with O.LaunchList.record() as ll:
            rc = LB.lib().llark_prior_attn(None, 0, 1, 64, 48, 2, 8, 1, None, None, 0, None)     # rejected before any HIP call
            assert rc == -1
            with pytest.raises(RuntimeError, match="does not nest"):
                O.LaunchList.record().__enter__()
        assert [c[1] for c in ll.calls] == ["llark_prior_attn"] and ll.calls[0][2][2:5] == (1, 64, 48)
        assert LB._recorder is None and not isinstance(LB.lib(), LB._RecordingProxy)
        with pytest.raises(LB.LlarkHipError, match="llark_prior_attn"):
            ll.replay()
    finally:
        import torch
        O._stream = lambda: torch.cuda.current_stream().cuda_stream


import pytest


@pytest.mark.gpu
def test_persistent_gemms_on_two_streams_use_separate_caller_owned_workspaces():
    """include/llark_hip.h: compute entry points keep no hidden device state -- the persistent GEMM kernels synchronise through
    a workspace the CALLER creates (llark_workspace_create), one per (device, stream).  Two streams run the persistent kernels
    (f16x2 variant 30 and the lo8 form) concurrently, each with its own workspace; results equal the single-stream run bit for
    bit, and the library allocates nothing after the two workspaces exist."""
    import torch

    from llark_amd import ops

    g = torch.Generator().manual_seed(0)
    m, n, k = 8192, 4800, 1216
    a = torch.randn(m, k, generator=g)
    w = (torch.randn(n, k, generator=g) * 0.02).half().cuda()
    hi, lo = ops.split16(a.cuda(), torch.float16, kmult=64)
    wt = torch.zeros((n, hi.shape[1]), dtype=torch.float16, device="cuda")
    wt[:, :k] = w
    lo8 = torch.randint(0, 120, (m, hi.shape[1]), dtype=torch.uint8, device="cuda")
    sw = ops.lo8_weight_exponent(wt)
    w8 = ops.pack_weight_lo8(wt, sw)

    def run(kind, out):
        if kind == 0:
            ops.gemm16(hi, lo, wt, None, n, ops.EPI_F32, c=out, variant=30)
        else:
            ops.gemm16_lo8(hi, lo8, wt, sw, None, n, ops.EPI_F32, c=out, w8=w8)

    ref = [torch.empty(m, n, device="cuda") for _ in range(2)]
    for kind in range(2):
        run(kind, ref[kind])
    torch.cuda.synchronize()
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    outs = {(i, kind): torch.empty(m, n, device="cuda") for i in range(2) for kind in range(2)}
    n_before = len(ops._workspaces)
    for rep in range(3):
        for i, st in enumerate((s1, s2)):
            with torch.cuda.stream(st):
                for kind in range(2):
                    run(kind, outs[(i, kind)])
    torch.cuda.synchronize()
    assert len(ops._workspaces) == n_before + 2                      # one workspace per new stream, created once
    ws = [ops._workspaces[(torch.cuda.current_device(), st.cuda_stream)] for st in (s1, s2)]
    assert ws[0] != ws[1]
    for (i, kind), o in outs.items():
        assert torch.equal(o, ref[kind]), f"stream {i}, kernel {kind}: result differs from the single-stream run"
    # without a workspace the plain entry point never runs a persistent variant, and says nothing else changed
    c = torch.empty(m, n, device="cuda")
    rc = _lib.lib().llark_gemm16_ex(30, 0, 1, 0, hi.data_ptr(), lo.data_ptr(), hi.stride(0), wt.data_ptr(), wt.stride(0), None, m, n,
                                    wt.shape[1], c.data_ptr(), c.stride(0), None, 0, None, None, 0, torch.cuda.current_stream().cuda_stream)
    assert rc == 0
    torch.cuda.synchronize()
    assert torch.equal(c, ref[0])                                    # every tile variant computes the same product
