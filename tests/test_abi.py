"""CPU: the C-ABI shared library exists in-tree, loads, and exports every symbol include/tmjx.h declares."""
import ctypes
import re
import subprocess
from pathlib import Path

from track_mjx_amd import hip

ROOT = Path(__file__).resolve().parents[1]


def _declared():
    text = (ROOT / "include" / "tmjx.h").read_text()
    return sorted(set(re.findall(r"\b(tmjx_[a-z0-9_]+)\s*\(", text)))


def test_header_symbols_are_exported():
    if not hip.SO_PATH.exists():
        hip.build()
    out = subprocess.run(["nm", "-D", "--defined-only", str(hip.SO_PATH)], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r"\bT (tmjx_[a-z0-9_]+)", out))
    declared = _declared()
    assert len(declared) >= 12
    assert not [s for s in declared if s not in exported], exported
    assert set(hip.EXPORTS) <= exported


def _ctype_kind(t):
    """A ctypes argument type as the header would spell its kind: "pointer", or (class, bytes) of a scalar."""
    if t in (ctypes.c_void_p, ctypes.c_char_p) or not isinstance(getattr(t, "_type_", ""), str):
        return "pointer"
    return ("float" if t._type_ in "fd" else "int", ctypes.sizeof(t))


def test_signature_table_agrees_with_the_header():
    """hip.SIGNATURES against the prototypes of include/tmjx.h, every tmjx_* function: the number of arguments, a pointer exactly where the header
    has one, the size and the integer / floating class of every scalar, and the return type.  No allow-list."""
    from tests.abi_header import SCALARS, prototypes
    protos = prototypes()
    assert sorted(protos) == _declared() and set(protos) == set(hip.SIGNATURES) and len(protos) >= 148
    returns = {"int": ctypes.c_int, "long long": ctypes.c_longlong, "char*": ctypes.c_char_p, "void": None}
    for name, (ret, args) in protos.items():
        argtypes, restype = hip.SIGNATURES[name]
        assert len(argtypes) == len(args), f"{name}: {len(argtypes)} argument types for {len(args)} parameters"
        for i, ((ctype, pname), t) in enumerate(zip(args, argtypes)):
            want = "pointer" if ctype.endswith("*") else SCALARS[ctype]
            assert _ctype_kind(t) == want, f"{name}: argument {i} ({ctype} {pname}) is declared {t.__name__}"
        same = restype is returns[ret] or (ret == "long long" and restype is not None and _ctype_kind(restype) == ("int", 8))      # (c_int64 is c_long)
        assert same, f"{name}: returns {ret}, declared {restype}"


def test_library_loads_and_reports_errors_without_gpu():
    L = hip.lib()
    assert b"gfx950" in L.tmjx_version()
    h = ctypes.c_void_p()
    assert L.tmjx_model_create(None, 0, ctypes.byref(h)) == -22       # TMJX_EINVAL, no compute call
    assert L.tmjx_last_error()


def test_no_product_import_of_oracle_or_emulation():
    """The product package must not reach into oracle/ or the host emulation (no CPU fallback)."""
    pat = re.compile(r"^\s*(from|import)\s+[\w.]*\b(oracle|hostemu|emu)\b", re.M)
    for p in (ROOT / "track_mjx_amd").rglob("*.py"):
        src = p.read_text()
        assert not pat.search(src), p
        assert "liboracle" not in src and "libhostemu" not in src, p


def test_chain_layout_fits_fourteen_envs_per_cu():
    """The rodent (chain) LDS map of the wave kernel must stay within 9 of the CU's 128 LDS granules of 1280 bytes (measured granule:
    tools/micro/lds_occupancy.hip): room for fourteen envs per CU (csrc/wave_layout.h; ten granules in round 4) — the register bound, not LDS, keeps
    the product at twelve (csrc/tmjx_wave.hip says why)."""
    import subprocess, tempfile, textwrap
    from pathlib import Path
    root = Path(__file__).resolve().parents[1]
    src = textwrap.dedent(f'''
        #include <cstdio>
        #include "{root}/track_mjx_amd/csrc/wave_layout.h"
        int main() {{ constexpr WLayout k(TMW_RODENT_DIMS, 1); constexpr WLayout g(TMW_RODENT_DIMS, 0);
          static_assert(k.m_spilled(), "chain layout shares the matrix region");
          printf("%d %d\\n", k.lds_floats, g.lds_floats); return 0; }}''')
    with tempfile.TemporaryDirectory() as d:
        (Path(d) / "l.cpp").write_text(src)
        subprocess.run(["g++", "-std=c++17", "-o", f"{d}/l", f"{d}/l.cpp"], check=True)
        chain, generic = (int(v) for v in subprocess.run([f"{d}/l"], check=True, capture_output=True, text=True).stdout.split())
    # LDS is granted in 1280-byte granules on gfx950 (tools/micro/lds_occupancy.hip): 9 granules = fourteen resident envs per CU (128 // 9)
    assert chain * 4 <= 9 * 1280 and generic * 4 <= 20 * 1024 + 2048


def test_physics_kernel_resources_allow_three_waves_per_simd(tmp_path):
    """The rodent physics kernel in the built library must keep <= 168 VGPRs (three waves per SIMD: 3 x 168 <= 512 = twelve envs per CU; it takes
    about 130 — the four-wave build at 128 registers was measured slower, csrc/tmjx_wave.hip), no spills and no scratch: 172 registers once
    silently cut the pipelined roll-out back to 8 envs per CU.  Read from the code object's metadata."""
    import shutil, subprocess
    from track_mjx_amd import hip
    bundler, readelf = "/opt/rocm/lib/llvm/bin/clang-offload-bundler", "/opt/rocm/lib/llvm/bin/llvm-readelf"
    if not (hip.SO_PATH.exists() and shutil.which("objcopy") and Path(bundler).exists() and Path(readelf).exists()):
        import pytest
        pytest.skip("library or LLVM tools missing")
    fat = tmp_path / "fat.bin"
    subprocess.run(["objcopy", "-O", "binary", "--only-section=.hip_fatbin", str(hip.SO_PATH), str(fat)], check=True)
    # one offload bundle per translation unit of the library (the physics kernel has its own: csrc/tmjx_wave.hip)
    blob, magic = fat.read_bytes(), b"__CLANG_OFFLOAD_BUNDLE__"
    starts = [m.start() for m in re.finditer(re.escape(magic), blob)] + [len(blob)]
    notes = ""
    for k in range(len(starts) - 1):
        part, co = tmp_path / f"fat{k}.bin", tmp_path / f"k{k}.co"
        part.write_bytes(blob[starts[k]:starts[k + 1]])
        subprocess.run([bundler, "--unbundle", "--type=o", f"--input={part}", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", f"--output={co}"], check=True)
        notes += subprocess.run([readelf, "--notes", str(co)], check=True, capture_output=True, text=True).stdout
    i = notes.index(".name:           _Z14k_physics_waveILb1EE")
    after = notes[i:i + 1500]          # the fields of a kernel's metadata map follow its .name line in alphabetical order
    vg = int(re.search(r"\.vgpr_count:\s+(\d+)", after).group(1))
    sp = int(re.search(r"\.vgpr_spill_count:\s+(\d+)", after).group(1))
    scratch = int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", after).group(1))
    # the occupancy-relevant bound: three waves per SIMD = floor(512 / 168) allocated VGPRs (__launch_bounds__(64, 3)); the kernel takes ~130 — reported,
    # not pinned: a compiler that lands anywhere up to 168 changes nothing about the residency
    print(f"k_physics_wave<true>: {vg} VGPRs (bound 168 = three waves per SIMD), {sp} spilled, {scratch} B scratch")
    assert vg <= 168 and sp == 0 and scratch == 0, (vg, sp, scratch)


def test_argument_validation_of_the_learner_entry_points_without_gpu():
    """Every entry point validates before it launches: null pointers, empty or inconsistent sizes and group counts return TMJX_EINVAL
    (-22) with a message — no compute call is made (runs in the GPU-less build container)."""
    L = hip.lib()
    vp = ctypes.c_void_p
    one = vp(16)            # a non-null, 16-byte aligned dummy that is never dereferenced: validation fails first
    assert L.tmjx_gemm_nt(None, 4, one, 4, None, one, 4, 1, 1, 1, None) == -22
    assert L.tmjx_gemm_nt(one, 4, one, 4, None, one, 4, 0, 4, 4, None) == -22            # M = 0: empty input
    assert L.tmjx_gemm_nt(one, 2, one, 4, None, one, 4, 4, 4, 4, None) == -22            # lda < K
    assert L.tmjx_gemm_nn(one, 4, one, 2, one, 4, 4, 4, 4, None) == -22                  # ldw < N
    assert L.tmjx_gemm_dw(one, 4, one, 4, None, None, one, 4, 4, 4, None) == -22
    assert L.tmjx_gemm_dw_scratch_floats(0, 4, 4) == 0 and L.tmjx_gemm_dw_scratch_floats(20480, 256, 256) > 0
    assert L.tmjx_gemm_dw_grouped(None, 1, None) == -22
    arr = (hip.DwProblem * 1)()
    assert L.tmjx_gemm_dw_grouped(arr, 0, None) == -22 and L.tmjx_gemm_dw_grouped(arr, 17, None) == -22
    assert L.tmjx_gemm_dw_grouped(arr, 1, None) == -22                                   # null pointers inside the problem
    arr[0] = hip.DwProblem(8, 16, 16, None, 16, 4, 4, 4, 4, 4, 4)                        # dY not 16-byte aligned
    assert L.tmjx_gemm_dw_grouped(arr, 1, None) == -22 and b"aligned" in L.tmjx_last_error()
    assert L.tmjx_stats_sums(one, one, one, one, 10, 6, None) == -22                     # W not a multiple of 4
    assert L.tmjx_stats_apply(one, 0.0, one, one, one, one, 4, 1e-6, 1e6, None) == -22   # n_added must be positive
    assert L.tmjx_set_wrappers(None, 195, 1) == -22
    assert L.tmjx_set_action_repeat(None, 2) == -22
    assert L.tmjx_last_error()


def test_argument_validation_of_the_chain_entry_points_without_gpu():
    """tmjx_chain_fwd / tmjx_chain_bwd (csrc/mlp_chain.h) validate before they launch: what a chain kernel cannot run — null pointers, hidden layers that are not 256
    wide, unaligned rows, a last layer wider than 128, y / dz buffers without the row-tile padding — is TMJX_EINVAL with a message, and the `_ok` twins say so
    without an error.  No compute call is made (GPU-less build container)."""
    L = hip.lib()
    a = 1 << 20                                                    # a non-null, 16-byte aligned dummy address that is never dereferenced

    def fwd(M=20480, K0=472, lda=696, n=2, Nf=120, rows=None, **over):
        d = hip.ChainFwd()
        d.A, d.lda, d.M, d.n_hidden, d.epi, d.eps = a, lda, M, n, 1, 1e-6
        for l in range(min(n, 4)):
            h = d.hidden[l]
            h.W, h.bias, h.gamma, h.beta, h.z, h.y, h.stats, h.K, h.ldw = a, a, a, a, a, a, a, (K0 if l == 0 else 256), (K0 if l == 0 else 256)
        d.Wf, d.bf, d.outf, d.Nf, d.ldwf, d.ldof = a, a, a, Nf, 256, Nf
        d.rows_alloc = L.tmjx_chain_rows(M) if rows is None else rows
        for k, v in over.items():
            setattr(d, k, v)
        return d
    assert L.tmjx_chain_rows(20480) == 20480 and L.tmjx_chain_rows(5120) == 5120 and L.tmjx_chain_rows(1365) % 32 == 0 and L.tmjx_chain_rows(1365) >= 1365
    assert L.tmjx_chain_rows(0) == 0
    assert L.tmjx_chain_fwd_ok(ctypes.byref(fwd())) == 1
    for bad, word in ((fwd(Nf=130), b"128"), (fwd(lda=695), b"aligned"), (fwd(rows=20479), b"rows_alloc"), (fwd(n=5), b"hidden"), (fwd(n=0), b"hidden"), (fwd(A=None), b"null"),
                      (fwd(epi=2), b"epi"), (fwd(M=0), b"M >= 1")):
        assert L.tmjx_chain_fwd_ok(ctypes.byref(bad)) == 0
        assert L.tmjx_chain_fwd(ctypes.byref(bad), None) == -22 and word in L.tmjx_last_error(), (word, L.tmjx_last_error())
    wide = fwd()
    wide.hidden[1].K, wide.hidden[1].ldw = 512, 512                # a hidden layer whose input is not 256 wide
    assert L.tmjx_chain_fwd(ctypes.byref(wide), None) == -22 and b"256" in L.tmjx_last_error()
    assert L.tmjx_chain_fwd(None, None) == -22

    def bwd(M=20480, Kg=76, n=2, epi=2, **over):
        d = hip.ChainBwd()
        d.G, d.ldg, d.Kg, d.M, d.n_stages, d.epi, d.rows_alloc = a, Kg, Kg, M, n, epi, L.tmjx_chain_rows(M)
        for i in range(min(n, 4)):
            s = d.stage[i]
            s.W, s.ldw, s.z, s.bias, s.gamma, s.stats, s.dz, s.partial = a, 256, a, a, a, a, a, a
        for k, v in over.items():
            setattr(d, k, v)
        return d
    assert L.tmjx_chain_bwd_ok(ctypes.byref(bwd())) == 1
    assert L.tmjx_chain_bwd_ok(ctypes.byref(bwd(W0=a, ldw0=288, dx_cols=60, dx=a, lddx=286))) == 1
    assert L.tmjx_chain_bwd_ok(ctypes.byref(bwd(Kg=1, epi=4, ldg=1))) == 1                     # the value head
    for bad, word in ((bwd(Kg=130), b"128"), (bwd(Kg=1), b"1-wide"), (bwd(epi=3), b"epi"), (bwd(rows_alloc=100), b"rows_alloc"), (bwd(n=0), b"stages"),
                      (bwd(Kg=78), b"aligned"), (bwd(W0=a, ldw0=288, dx_cols=200, dx=a, lddx=286), b"trailing"), (bwd(G=None), b"null")):
        assert L.tmjx_chain_bwd_ok(ctypes.byref(bad)) == 0
        assert L.tmjx_chain_bwd(ctypes.byref(bad), None) == -22 and word in L.tmjx_last_error(), (word, L.tmjx_last_error())
