"""CPU suite: the drop-in boundary.  The C-ABI library loads, exports exactly what the headers under include/ declare, the
Python binding mirrors them name by name and type by type, the product never touches the oracle, and it fails loudly - no
CPU fallback - when asked to compute without a GPU."""
import ctypes
import pathlib
import re

import pytest
import torch

ROOT = pathlib.Path(__file__).resolve().parent.parent

# The entry points each header is expected to declare, pinned here so that one cannot come or go unnoticed.
EXPECTED = {
    "artist_hip.h": [
        "art_abi_version", "art_last_hip_error", "art_strerror", "art_trace_fwd", "art_trace_bwd",
        "art_per_target_sum", "art_nurbs_fwd", "art_nurbs_bwd", "art_align_fwd", "art_align_bwd", "art_reflect",
        "art_blocking_filter", "art_blocking_workspace_bytes", "art_flux_crop_fwd", "art_flux_crop_bwd",
        "art_flux_loss", "art_rigid_body_fwd", "art_rigid_body_bwd", "art_async_status", "art_trace_bwd_scratch_floats",
        "art_trace_bwd_scratch_need", "art_adam_step",
        "art_flux_crop_pixel_loss_fwd", "art_flux_crop_pixel_loss_bwd", "art_flux_crop_kl_loss_fwd",
        "art_flux_crop_kl_loss_bwd", "art_flux_center_of_mass", "art_flux_center_of_mass_bwd"],
    "artist_hip_sampler.h": ["art_sample_distortions", "art_sample_radial_distortions"],
    "artist_hip_regularizers.h": ["art_surface_regularizers_fwd", "art_surface_regularizers_bwd"],
    "artist_hip_surface_fit.h": ["art_surface_fit_table_words", "art_surface_fit_prepare", "art_surface_fit_loss_grad",
                                 "art_surface_fit_run"],
    "artist_hip_canting.h": ["art_cant_facets_fwd", "art_cant_facets_bwd"],
    "artist_hip_shading.h": ["art_shading_cull", "art_shading_prims_fwd", "art_shading_prims_bwd", "art_shading_append"],
}
HEADERS = sorted(path.name for path in (ROOT / "include").glob("*.h"))
# The only ART_ macros outside artist_hip.h: values of an argument (surface fitting's `mode`), not return codes.
OTHER_DEFINES = {"artist_hip_surface_fit.h": ["ART_FIT_NORMALS", "ART_FIT_POINTS"]}

# C type -> ctypes type, by kind: every pointer travels as c_void_p; a pointer is a return type only as `const char *`
PARAMETER_KINDS = {"int64_t": ctypes.c_int64, "int": ctypes.c_int, "double": ctypes.c_double, "float": ctypes.c_float}
RETURN_KINDS = {"int": ctypes.c_int, "int64_t": ctypes.c_int64, "const char *": ctypes.c_char_p}


def header_text(header):
    return re.sub(r"/\*.*?\*/", "", (ROOT / "include" / header).read_text(), flags=re.S)


def header_functions(header="artist_hip.h"):
    return sorted(set(re.findall(r"\b(art_[a-z_0-9]+)\s*\(", header_text(header))))


def header_prototypes(header):
    """name -> (restype, [argtypes]) as the header declares them, in ctypes terms."""
    protos = {}
    for ret, name, params in re.findall(r"^((?:const\s+)?\w+\s*\*?)\s*(art_\w+)\s*\(([^)]*)\)\s*;", header_text(header), flags=re.M):
        # a parameter without a star is "[const] type name"
        argtypes = [ctypes.c_void_p if "*" in param else PARAMETER_KINDS[" ".join(w for w in param.split()[:-1] if w != "const")]
                    for param in ([] if params.strip() in ("", "void") else params.split(","))]
        assert name not in protos, name
        protos[name] = (RETURN_KINDS[" ".join(ret.replace("*", " * ").split())], argtypes)
    return protos


def test_header_declares_the_expected_entry_points():
    assert header_functions() == sorted(EXPECTED["artist_hip.h"])


@pytest.mark.parametrize("header", HEADERS)
def test_binding_mirrors_the_header(header):
    """Names, exports, and - by kind - every parameter and return type: an ``int`` bound where the header says ``int64_t``, or a
    pointer where it says ``double``, corrupts arguments on the way to the device instead of raising.  The public headers are
    the files directly under include/: no entry point is declared in two of them, and the return codes are artist_hip.h's."""
    from artist_amd import _lib
    assert sorted(_lib.HEADERS) == HEADERS == sorted(EXPECTED)
    assert [path for path in (ROOT / "include").rglob("*.h") if path.parent != ROOT / "include"] == []
    declared = [name for h in HEADERS for name in header_functions(h)]
    assert len(declared) == len(set(declared)), sorted(name for name in set(declared) if declared.count(name) > 1)
    if header != "artist_hip.h":
        assert sorted(re.findall(r"#define\s+(ART_\w+)", header_text(header))) == OTHER_DEFINES.get(header, [])
        assert '#include "artist_hip.h"' in header_text(header)
    assert sum(len(names) for names in _lib.HEADERS.values()) == len(_lib.SIGNATURES)          # no name under two headers
    assert {name for names in _lib.HEADERS.values() for name in names} == set(_lib.SIGNATURES)
    protos = header_prototypes(header)
    assert protos and sorted(protos) == header_functions(header) == sorted(_lib.HEADERS[header]) == sorted(EXPECTED[header])
    exported = ctypes.CDLL(str(_lib.LIB_PATH))
    lib = _lib.lib()                       # no compute call: loading + version query only
    for name, (restype, argtypes) in protos.items():
        assert hasattr(exported, name), f"{name} missing from {_lib.LIB_PATH}"
        assert _lib.SIGNATURES[name] == (restype, argtypes), name
        bound = getattr(lib, name)
        assert (bound.restype, list(bound.argtypes)) == (restype, argtypes), name
    # the return codes: every ART_OK / ART_E* the headers define, with the header's value
    defines = {name: int(value) for h in HEADERS
               for name, value in re.findall(r"^#define (ART_OK|ART_E\w+) (-?\d+)", header_text(h), flags=re.M)}
    assert defines == {name: value for name, value in vars(_lib).items() if name == "ART_OK" or name.startswith("ART_E")}
    assert sorted(defines) == sorted(["ART_OK", "ART_EINVAL", "ART_ETARGET", "ART_ELAUNCH", "ART_EUNSUPPORTED", "ART_ECANDIDATES",
                                      "ART_EQUEUE"])
    assert lib.art_abi_version() == _lib.ABI_VERSION == 13
    assert lib.art_strerror(_lib.ART_OK) == b"ok" and b"invalid" in lib.art_strerror(_lib.ART_EINVAL)


def test_product_does_not_touch_the_oracle():
    for path in (ROOT / "artist_amd").rglob("*"):
        if path.suffix in {".py", ".hip", ".hpp", ".h", ".cpp"} or path.name == "Makefile":
            text = path.read_text()
            assert "oracle" not in text.lower() or path.name == "_never_", f"{path} mentions the oracle"


def test_no_cpu_fallback():
    from artist_amd import ArtistHipError, NURBSSurfaces, trace_rays
    z = torch.zeros
    with pytest.raises(ArtistHipError, match="no CPU fallback"):
        trace_rays(z(1, 4, 4), z(1, 4, 4), z(1, 4), z(1, 2, 4), z(1, 2, 4), z(1, dtype=torch.long), z(1, 4), z(1, 4),
                   torch.ones(1, 2))
    surf = NURBSSurfaces(torch.tensor([3, 3]), torch.rand(1, 1, 6, 6, 3), device=torch.device("cpu"))
    with pytest.raises(ArtistHipError, match="no CPU fallback"):
        surf(torch.rand(1, 1, 5, 2), None, None)


def test_missing_library_is_an_error(monkeypatch, tmp_path):
    from artist_amd import _lib
    monkeypatch.setattr(_lib, "_LIB", None)
    monkeypatch.setattr(_lib, "LIB_PATH", tmp_path / "libartist_hip.so")
    with pytest.raises(_lib.ArtistHipError, match="no CPU fallback"):
        _lib.lib()


def test_no_float_atomics_in_any_trace_kernel(tmp_path):
    """Determinism by construction: the device code of libartist_hip.so holds no float atomic - neither
    `global_atomic_add_f32` nor an LDS `ds_add_f32` / `ds_add_f64` (`ds_add_rtn_*` likewise) - in ANY trace kernel, planar
    or cylindrical, blocking on or off: flux goes through 64-bit integer accumulators, gradients through plain stores and
    chunk slabs, and the rectangle gradients of the blocking backward through wave reductions and item slabs (round 2
    still flushed those with float atomics) - with one narrow exception since round 4, stated where it is checked below."""
    import shutil
    import subprocess
    llvm = pathlib.Path("/opt/rocm/lib/llvm/bin")
    if not (llvm / "llvm-objdump").exists() or not (llvm / "clang-offload-bundler").exists():
        pytest.skip("ROCm LLVM tools not installed")
    lib = ROOT / "artist_amd" / "libartist_hip.so"
    fat = tmp_path / "fat.bin"
    subprocess.run([str(llvm / "llvm-objcopy"), "--dump-section", f".hip_fatbin={fat}", str(lib), str(tmp_path / "stripped.so")], check=True)
    blob = fat.read_bytes()
    magic = b"__CLANG_OFFLOAD_BUNDLE__"
    starts = [m.start() for m in re.finditer(re.escape(magic), blob)]
    assert starts, "no offload bundles in the library"
    per_kernel, per_kernel_f64_only, seen_trace = {}, {}, False

    def blocking_instantiation(mangled):
        # trace_bwd_lds_kernel<INTERLEAVED, ATOMIC_OUT, CYL, BLOCKING, LEAN>: the fourth template argument
        dem = subprocess.run(["c++filt", mangled], capture_output=True, text=True).stdout
        m = re.search(r"trace_bwd_lds_kernel<(\w+), (\w+), (\w+), (\w+), (\w+)>", dem)
        return bool(m) and m.group(4) == "true"
    for k, start in enumerate(starts):
        part = tmp_path / f"bundle{k}.bin"
        part.write_bytes(blob[start: starts[k + 1] if k + 1 < len(starts) else len(blob)])
        code = tmp_path / f"code{k}.co"
        subprocess.run([str(llvm / "clang-offload-bundler"), "--unbundle", "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950",
                        f"--input={part}", f"--output={code}"], check=True)
        if not code.exists() or code.stat().st_size == 0:
            continue
        text = subprocess.run([str(llvm / "llvm-objdump"), "-d", str(code)], check=True, capture_output=True, text=True).stdout
        current = None
        for line in text.splitlines():
            m = re.match(r"^[0-9a-f]+ <(\w+)>:", line)
            if m:
                current = m.group(1)
                seen_trace |= "trace_fwd_lds_kernel" in current
            elif current and re.search(r"global_atomic_(add|pk_add)_f(32|64)|ds_(add|pk_add)(_rtn)?_f(32|64)", line):
                per_kernel[current] = per_kernel.get(current, 0) + 1
                only_f64 = re.search(r"global_atomic_add_f64", line) is not None
                per_kernel_f64_only[current] = per_kernel_f64_only.get(current, True) and only_f64
    assert seen_trace, "trace kernels not found in the device code"
    offenders = {k: v for k, v in per_kernel.items() if "trace_" in k or "reduce_prim" in k or "reduce_chunks" in k}
    # The one exception (round 4): the blocking BACKWARD kernels add the rectangle gradients of a "wide" heliostat's listed
    # candidates - the ones beyond the 32 of the LDS tables - to its fp64 row by global fp64 atomics.  No other float atomic
    # anywhere: not in the forward kernels, not in the kernels without blocking, none on fp32, none in LDS.
    allowed = {k for k in offenders if "trace_bwd_lds_kernel" in k and per_kernel_f64_only.get(k, False) and blocking_instantiation(k)}
    assert not (set(offenders) - allowed), {k: offenders[k] for k in set(offenders) - allowed}
    assert not any("trace_fwd" in k for k in offenders)
