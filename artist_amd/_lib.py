"""ctypes binding of ``libartist_hip.so`` (C ABI declared in the headers under ``include/``).

The HIP library is the product path and there is no fallback: if the shared object is missing
or fails to load, importing any op raises ``ArtistHipError`` - loudly - instead of silently
computing on the CPU.
"""
from __future__ import annotations

import ctypes
import os
import pathlib
import subprocess

import torch  # before the library is loaded: see lib()

_PKG = pathlib.Path(__file__).resolve().parent
LIB_PATH = pathlib.Path(os.environ.get("ARTIST_HIP_LIB", _PKG / "libartist_hip.so"))   # override: diagnostic builds only
CSRC = _PKG / "csrc"

ABI_VERSION = 13


class ArtistHipError(RuntimeError):
    """Raised when libartist_hip.so is unavailable or an entry point reports an error."""


_c_i64 = ctypes.c_int64
_c_int = ctypes.c_int
_c_dbl = ctypes.c_double
_c_flt = ctypes.c_float
_c_str = ctypes.c_char_p
_ptr = ctypes.c_void_p

# Return codes of the entry points (include/artist_hip.h).
ART_OK = 0
ART_EINVAL = -1
ART_ETARGET = -2
ART_ELAUNCH = -3
ART_EUNSUPPORTED = -4
ART_ECANDIDATES = -5
ART_EQUEUE = -6

# header under include/ -> entry point -> (restype, argtypes): mirrors the declarations one-to-one
# (tests/test_boundary.py compares every name, parameter and return type with the headers).
_BY_HEADER = {
    "artist_hip.h": {
        "art_trace_fwd": (_c_int, [_ptr, _ptr, _ptr, _ptr, _ptr, _c_i64, _c_i64, _c_i64, _ptr, _ptr, _ptr, _ptr,
                                   _ptr, _ptr, _ptr, _ptr, _ptr, _ptr,
                                   _ptr, _ptr, _ptr, _ptr, _ptr, _c_i64, _c_dbl,
                                   _c_dbl, _c_dbl, _c_dbl, _c_i64, _c_i64, _c_i64, _c_i64, _c_i64, _c_i64, _c_i64, _c_i64, _c_int,
                                   _ptr, _ptr, _ptr, _ptr, _ptr]),
        "art_async_status": (_c_int, [_ptr, _c_int]),
        "art_trace_bwd": (_c_int, [_ptr, _ptr, _ptr, _ptr, _ptr, _c_i64, _c_i64, _c_i64, _ptr, _ptr, _ptr, _ptr,
                                   _ptr, _ptr, _ptr, _ptr, _ptr, _ptr,
                                   _ptr, _ptr, _ptr, _ptr, _ptr, _c_i64, _c_i64, _c_dbl,
                                   _c_dbl, _c_dbl, _c_dbl, _c_i64, _c_i64, _c_i64, _c_i64, _c_i64, _c_i64, _c_i64, _c_i64, _c_int,
                                   _ptr, _ptr, _ptr, _ptr, _ptr, _ptr, _ptr, _c_i64, _ptr]),
        "art_trace_bwd_scratch_floats": (_c_i64, [_c_i64, _c_i64, _c_i64, _c_i64, _c_i64]),
        "art_trace_bwd_scratch_need": (_c_i64, [_c_i64, _c_i64, _c_i64, _c_i64, _c_i64, _c_i64, _c_i64]),
        "art_flux_crop_fwd": (_c_int, [_ptr, _ptr, _c_i64, _c_i64, _c_i64, _c_dbl, _c_dbl, _ptr, _ptr, _ptr]),
        "art_flux_crop_bwd": (_c_int, [_ptr, _ptr, _ptr, _c_i64, _c_i64, _c_i64, _c_dbl, _c_dbl, _ptr, _ptr, _ptr, _ptr]),
        "art_flux_loss": (_c_int, [_ptr, _ptr, _c_i64, _c_i64, _c_int, _ptr, _ptr, _ptr, _ptr]),
        "art_flux_crop_pixel_loss_fwd": (_c_int, [_ptr, _ptr, _ptr, _c_i64, _c_i64, _c_i64, _c_dbl, _c_dbl, _ptr, _ptr, _ptr, _ptr, _ptr, _ptr]),
        "art_flux_crop_pixel_loss_bwd": (_c_int, [_ptr, _ptr, _ptr, _c_i64, _ptr, _ptr, _c_i64, _c_i64, _c_i64, _c_dbl, _c_dbl, _ptr, _ptr]),
        "art_flux_crop_kl_loss_fwd": (_c_int, [_ptr, _ptr, _ptr, _c_i64, _c_i64, _c_i64, _c_dbl, _c_dbl, _ptr, _ptr, _ptr]),
        "art_flux_crop_kl_loss_bwd": (_c_int, [_ptr, _ptr, _ptr, _ptr, _ptr, _c_i64, _c_i64, _c_i64, _c_dbl, _c_dbl, _ptr, _ptr, _ptr]),
        "art_flux_center_of_mass": (_c_int, [_ptr, _c_i64, _c_i64, _c_i64, _ptr, _ptr]),
        "art_flux_center_of_mass_bwd": (_c_int, [_ptr, _ptr, _c_i64, _c_i64, _c_i64, _ptr, _ptr]),
        "art_rigid_body_fwd": (_c_int, [_c_int, _ptr, _ptr, _ptr, _ptr, _c_i64, _ptr, _ptr, _ptr, _ptr, _c_i64, _c_int, _c_dbl,
                                        _ptr, _ptr, _ptr, _ptr, _ptr]),
        "art_rigid_body_bwd": (_c_int, [_c_int, _ptr, _ptr, _ptr, _ptr, _c_i64, _ptr, _ptr, _ptr, _ptr, _c_i64, _ptr, _ptr, _ptr,
                                        _ptr, _ptr, _ptr, _ptr, _ptr]),
        "art_blocking_workspace_bytes": (_c_i64, [_c_i64, _c_i64]),
        "art_blocking_filter": (_c_int, [_ptr, _ptr, _ptr, _ptr, _ptr, _c_i64, _c_i64, _c_i64, _ptr, _ptr, _ptr, _ptr,
                                         _ptr, _ptr, _ptr, _ptr, _ptr, _ptr, _c_dbl,
                                         _c_i64, _c_i64, _c_i64, _c_i64, _c_i64, _c_i64, _c_i64,
                                         _ptr, _ptr, _c_i64, _c_dbl, _c_int, _c_i64, _ptr, _ptr, _ptr, _ptr, _ptr]),
        "art_per_target_sum": (_c_int, [_ptr, _ptr, _c_i64, _c_i64, _c_i64, _ptr, _ptr]),
        "art_nurbs_fwd": (_c_int, [_ptr, _ptr, _c_i64, _c_i64, _ptr, _ptr, _ptr, _ptr, _c_int, _c_int, _c_int, _c_i64, _c_i64,
                                   _c_i64, _c_i64, _c_i64, _c_i64, _c_i64, _ptr, _ptr, _ptr, _ptr]),
        "art_nurbs_bwd": (_c_int, [_ptr, _ptr, _c_i64, _c_i64, _ptr, _ptr, _ptr, _c_int, _c_int, _c_int, _c_i64, _c_i64,
                                   _c_i64, _c_i64, _c_i64, _c_i64, _c_i64, _ptr, _ptr, _ptr, _ptr, _ptr]),
        "art_reflect": (_c_int, [_ptr, _ptr, _c_i64, _c_i64, _ptr, _ptr]),
        "art_adam_step": (_c_int, [_ptr, _ptr, _ptr, _ptr, _c_i64, _c_dbl, _c_dbl, _c_dbl, _c_dbl, _c_dbl, _c_i64, _c_int, _c_i64, _c_i64, _ptr]),
        "art_align_fwd": (_c_int, [_ptr, _ptr, _ptr, _c_i64, _c_i64, _ptr, _ptr, _ptr]),
        "art_align_bwd": (_c_int, [_ptr, _ptr, _ptr, _ptr, _ptr, _c_i64, _c_i64, _ptr, _ptr, _ptr, _ptr]),
        "art_abi_version": (_c_int, []),
        "art_last_hip_error": (_c_int, []),
        "art_strerror": (_c_str, [_c_int]),
    },
    "artist_hip_sampler.h": {
        "art_sample_distortions": (_c_int, [_c_i64, _ptr, _c_i64, _c_i64, _c_i64, _c_flt, _c_flt, _c_flt, _c_flt, _c_flt, _ptr, _ptr]),
        "art_sample_radial_distortions": (_c_int, [_c_i64, _ptr, _c_i64, _c_i64, _c_i64, _c_flt, _c_flt, _ptr, _c_i64, _ptr, _ptr]),
    },
    "artist_hip_regularizers.h": {
        "art_surface_regularizers_fwd": (_c_int, [_ptr, _ptr, _c_i64, _c_i64, _c_i64, _ptr, _ptr, _ptr]),
        "art_surface_regularizers_bwd": (_c_int, [_ptr, _ptr, _c_i64, _c_i64, _c_i64, _ptr, _ptr, _ptr, _ptr]),
    },
    "artist_hip_surface_fit.h": {
        "art_surface_fit_table_words": (_c_i64, [_c_int, _c_int]),
        "art_surface_fit_prepare": (_c_int, [_ptr, _ptr, _ptr, _ptr, _c_i64, _c_i64, _c_i64, _c_i64, _c_int, _c_int, _ptr, _ptr, _ptr, _ptr, _ptr, _ptr]),
        "art_surface_fit_loss_grad": (_c_int, [_ptr, _ptr, _ptr, _ptr, _ptr, _ptr, _c_i64, _c_i64, _c_i64, _c_i64, _c_int, _c_int, _c_int,
                                               _ptr, _ptr, _ptr, _ptr, _ptr]),
        "art_surface_fit_run": (_c_int, [_ptr, _ptr, _ptr, _ptr, _ptr, _ptr, _ptr, _ptr, _ptr, _ptr, _ptr, _c_i64, _c_i64, _c_i64, _c_i64,
                                         _c_int, _c_int, _c_int, _c_i64, _c_dbl, _c_i64, _c_dbl, _c_dbl, _c_dbl, _c_dbl, _c_int, _c_int, _c_int,
                                         _c_dbl, _c_i64, _c_dbl, _c_int, _c_i64, _c_dbl, _c_dbl, _ptr]),
    },
    "artist_hip_canting.h": {
        "art_cant_facets_fwd": (_c_int, [_ptr, _ptr, _ptr, _ptr, _c_int, _c_i64, _c_i64, _ptr, _ptr, _ptr]),
        "art_cant_facets_bwd": (_c_int, [_ptr, _ptr, _ptr, _ptr, _ptr, _c_int, _c_i64, _c_i64, _ptr, _ptr, _ptr, _ptr, _ptr]),
    },
    "artist_hip_shading.h": {
        "art_shading_cull": (_c_int, [_ptr, _ptr, _ptr, _c_i64, _c_i64, _c_dbl, _c_i64, _ptr, _ptr, _ptr]),
        "art_shading_prims_fwd": (_c_int, [_ptr, _ptr, _ptr, _ptr, _c_i64, _c_i64, _c_i64, _ptr, _ptr, _ptr, _ptr]),
        "art_shading_prims_bwd": (_c_int, [_ptr, _ptr, _ptr, _ptr, _ptr, _ptr, _ptr, _c_i64, _c_i64, _c_i64, _ptr, _ptr, _ptr]),
        "art_shading_append": (_c_int, [_ptr, _ptr, _c_i64, _c_i64, _c_i64, _c_i64, _ptr, _ptr, _ptr]),
    },
}

SIGNATURES = {name: signature for table in _BY_HEADER.values() for name, signature in table.items()}
HEADERS = {header: tuple(table) for header, table in _BY_HEADER.items()}

_LIB = None


def build(verbose: bool = False) -> pathlib.Path:
    """Compile every HIP source for gfx950 into artist_amd/libartist_hip.so (in-tree)."""
    cmd = ["make", "-C", str(CSRC), "-j", str(min(8, os.cpu_count() or 1))]
    res = subprocess.run(cmd, capture_output=not verbose, text=True)
    if res.returncode != 0:
        raise ArtistHipError(f"building libartist_hip.so failed:\n{res.stdout}\n{res.stderr}")
    if not LIB_PATH.exists():
        raise ArtistHipError(f"build finished but {LIB_PATH} is missing")
    return LIB_PATH


def bind(handle: ctypes.CDLL, path) -> ctypes.CDLL:
    """Give every entry point of ``SIGNATURES`` its types on ``handle`` (a build of the library loaded from ``path``) and check the
    ABI version."""
    for name, (restype, argtypes) in SIGNATURES.items():
        try:
            fn = getattr(handle, name)
        except AttributeError as exc:
            raise ArtistHipError(f"{path} does not export {name}") from exc
        fn.restype, fn.argtypes = restype, argtypes
    if handle.art_abi_version() != ABI_VERSION:
        raise ArtistHipError(f"ABI mismatch: library {handle.art_abi_version()} vs binding {ABI_VERSION}")
    return handle


def lib() -> ctypes.CDLL:
    """Load the library (once).  torch is imported first (at the top of this module) so that the HIP runtime already in
    the process (torch/lib/libamdhip64.so, soname libamdhip64.so.7) is the one our DT_NEEDED
    entry resolves to - two HIP runtimes in one process cannot share streams or allocations."""
    global _LIB
    if _LIB is not None:
        return _LIB
    if not LIB_PATH.exists():
        raise ArtistHipError(
            f"{LIB_PATH} not found. Build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            f"or `make -C {CSRC}`. There is no CPU fallback.")
    try:
        handle = ctypes.CDLL(str(LIB_PATH))
    except OSError as exc:  # pragma: no cover - depends on the host
        raise ArtistHipError(f"cannot load {LIB_PATH}: {exc}") from exc
    _LIB = bind(handle, LIB_PATH)
    return _LIB


def check(code: int, what: str) -> None:
    if code != ART_OK:
        handle = lib()
        msg = handle.art_strerror(code).decode()
        raise ArtistHipError(f"{what}: {msg} (code {code}, hipError {handle.art_last_hip_error()})")


def capturing() -> bool:
    """Is the current stream being captured into a graph (``torch.cuda.graph``)?  Asked where a cache misses or a call
    fails, never on a path that an epoch takes every time."""
    return torch.cuda.is_initialized() and torch.cuda.is_current_stream_capturing()


# Tensors that the package's caches handed to a step while artist_amd.graphs.EpochGraph captured it: their addresses are
# baked into the graph, but a cache may drop its entry (a bounded table, a new version of its key, an error that clears the
# accumulators) long before the graph is gone.  The graph keeps them.  None: nobody is capturing.
_KEPT_BY_CAPTURE = None


def keep_alive(*tensors) -> None:
    """Called by the caches on the tensors they hand out (one comparison when no EpochGraph is capturing)."""
    if _KEPT_BY_CAPTURE is not None:
        _KEPT_BY_CAPTURE.extend(t for t in tensors if t is not None)


def first_use_under_capture(what: str) -> ArtistHipError:
    """The error for state that would have to be created, zero-initialised or read back on the host while the stream
    is being captured - library memory, an accumulator buffer, a cache entry that needs a host read.  Nothing has been
    created and no HIP call has failed: the capture itself is still valid."""
    return ArtistHipError(f"{what}: first use on this stream under graph capture: run the step once on this stream before "
                          "capturing (artist_amd.graphs.EpochGraph does)")


def call(name: str, device, *args, on_error=check) -> None:
    """Launch entry point ``name`` on the current stream of ``device``, which goes in as the last argument (``void *stream``
    ends every launching entry point), and hand a non-zero return code to ``on_error(code, name)``.  The function is looked
    up on the handle at call time: tests wrap attributes of the handle and must see every call."""
    with torch.cuda.device(device):
        code = getattr(lib(), name)(*args, torch.cuda.current_stream(device).cuda_stream)
        if code == ART_EUNSUPPORTED and capturing():
            # the library creates nothing while its stream is being captured (include/artist_hip.h, Conventions)
            raise first_use_under_capture(name)
    if code != ART_OK:
        on_error(code, name)


def loaded_hip_runtimes() -> list[str]:
    """Paths of libamdhip64 images mapped into this process (must be exactly one)."""
    paths = set()
    with open("/proc/self/maps") as f:
        for line in f:
            if "libamdhip64" in line:
                paths.add(line.split()[-1])
    return sorted(paths)
