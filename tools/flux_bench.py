#!/usr/bin/env python3
"""The flux epilogue's ten entry points (artist_amd/csrc/flux_kernels.hip; art_flux_loss at each of its six kinds), timed or compared
bit for bit between builds.

Timing: bitmaps of 256 x 256 (default 1000, the metric field; 125 is one rank's share), every library loaded into ONE process and
timed in interleaved rounds - boxes differ by 10-20 % on the same binary, so only numbers of one run compare.  Per library and
call: median, minimum and maximum over the rounds, and the algorithmic HBM rate of the median (one read + one write of the bitmaps, two
reads for kernels with two inputs).  One JSON line per bitmap count.

--bits A=lib.so B=lib.so: every entry point of the two libraries on the inputs of tests/flux_ref.py (all of CASES) and on the metric
shape; per case, call and output buffer (results, records and the workspaces a caller reads) whether the bytes are equal.  The
fused pixel pair runs with ARTIST_HIP_LOSS_PARTS unset, 1, 2 and 4, with and without the centre-of-mass sums handed over.

usage:  python tools/flux_bench.py [BITMAPS ...] [--rounds 7] [--steps 20] [--out FILE] [NAME=path/to/lib.so ...]
        python tools/flux_bench.py --bits [--out FILE] A=path/to/lib.so B=path/to/lib.so
        (no NAME=: the built artist_amd/libartist_hip.so; a bare NAME= is that library too - twice, it gives the box's A/A spread)
"""
import argparse
import ctypes
import json
import os
import pathlib
import statistics
import sys

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

import torch  # noqa: E402

from artist_amd import _lib  # noqa: E402

DEV = torch.device("cuda:0")


def metric_inputs(B, Hh=256, W=256):
    g = torch.Generator(device=DEV).manual_seed(1)
    yy, xx = torch.meshgrid(torch.arange(Hh, device=DEV), torch.arange(W, device=DEV), indexing="ij")
    cx = W / 2 + 40 * torch.rand(B, 1, 1, device=DEV, generator=g) - 20
    cy = Hh / 2 + 40 * torch.rand(B, 1, 1, device=DEV, generator=g) - 20
    flux = torch.exp(-((xx - cx) ** 2 + (yy - cy) ** 2) / (2 * 18.0 ** 2)).contiguous()
    return dict(flux=flux, dims=torch.full((B, 2), 8.0, device=DEV), truth=torch.rand(B, Hh, W, device=DEV, generator=g) + 0.1,
                grad_out=torch.rand(B, Hh, W, device=DEV, generator=g), w=torch.ones(B, device=DEV),
                grad_com=torch.rand(B, 2, device=DEV, generator=g)), 6.0, 6.0


def moments_of(flux):
    """The centre-of-mass sums [B,4,3] as the trace's conversion pass hands them over (include/artist_hip.h `moments`), in torch fp64."""
    B, Hh, W = flux.shape
    lin = lambda k: torch.linspace(-1, 1, k, device=DEV, dtype=torch.float64)
    f64 = flux.double()
    parts = []
    for v in range(4):
        q, y = f64[:, (Hh * v) // 4:(Hh * (v + 1)) // 4], lin(Hh)[(Hh * v) // 4:(Hh * (v + 1)) // 4]
        parts.append(torch.stack([q.sum((1, 2)), (q * lin(W)[None, None, :]).sum((1, 2)), (q * y[None, :, None]).sum((1, 2))], 1))
    return torch.stack(parts, 1).contiguous()


def make_calls(inp, crop_w, crop_h):
    """[(name, fn(lib), names of the buffers it writes, algorithmic bytes)] in an order in which every call finds the records of
    the forward call before it, and the buffers by name."""
    flux, dims, truth, gout, gl, gcomp = (inp[k] for k in ("flux", "dims", "truth", "grad_out", "w", "grad_com"))
    B, Hh, W = flux.shape
    n = B * Hh * W * 4
    new = lambda *shape: torch.empty(*shape, device=DEV)
    buf = dict(crop=new(B, Hh, W), centers=new(B, 3), grad_flux=new(B, Hh, W), crop_ws=new(B, 3), loss=new(B), grad_pred=new(B, Hh, W),
               centers4=new(B, 4), residual=new(B, Hh, W), center_grad_unit=new(B, 2), record8=new(B, 8), kl_ws=new(B * Hh * W + 5 * B),
               com=new(B, 3), moments=moments_of(flux))
    s = torch.cuda.current_stream().cuda_stream
    p = lambda name: (buf[name] if isinstance(name, str) else name).data_ptr()
    cw, ch = crop_w, crop_h
    calls = [("crop_fwd", lambda L: L.art_flux_crop_fwd(p(flux), p(dims), B, Hh, W, cw, ch, p("crop"), p("centers"), s), ["crop", "centers"], 2 * n),
             ("crop_bwd", lambda L: L.art_flux_crop_bwd(p(flux), p(dims), p("centers"), B, Hh, W, cw, ch, p(gout), p("grad_flux"), p("crop_ws"), s),
              ["grad_flux", "crop_ws"], 3 * n)]
    for kind, tag in ((0, "pixel"), (1, "kl"), (2, "jensen_shannon"), (3, "shape_pixel"), (4, "total_variation"), (5, "cosine")):
        calls += [(f"{tag}_loss_fwd", lambda L, kind=kind: L.art_flux_loss(p("crop"), p(truth), B, Hh * W, kind, p("loss"), None, None, s), ["loss"], 2 * n),
                  (f"{tag}_loss_bwd", lambda L, kind=kind: L.art_flux_loss(p("crop"), p(truth), B, Hh * W, kind, None, p(gl), p("grad_pred"), s),
                   ["grad_pred"], 3 * n)]
    fused = lambda keep, m: lambda L: L.art_flux_crop_pixel_loss_fwd(p(flux), p(dims), p(truth), B, Hh, W, cw, ch, p("loss"), p("centers4"),
                                                                      p("residual") if keep else None, p("center_grad_unit") if keep else None, m, s)
    calls += [("crop_pixel_loss_fwd", fused(False, None), ["loss", "centers4"], 2 * n),
              ("crop_pixel_loss_fwd_keep_moments", fused(True, p("moments")), ["loss", "centers4", "residual", "center_grad_unit"], 3 * n),
              ("crop_pixel_loss_fwd_keep", fused(True, None), ["loss", "centers4", "residual", "center_grad_unit"], 3 * n)]
    for stride in (1, 0):           # (0: the gradient of a summed loss)
        calls.append((f"crop_pixel_loss_bwd{'' if stride else '_stride0'}",
                      lambda L, stride=stride: L.art_flux_crop_pixel_loss_bwd(p(dims), p("centers4"), p(gl), stride, p("residual"), p("center_grad_unit"),
                                                                              B, Hh, W, cw, ch, p("grad_flux"), s), ["grad_flux"], 2 * n))
    calls += [("crop_kl_loss_fwd", lambda L: L.art_flux_crop_kl_loss_fwd(p(flux), p(dims), p(truth), B, Hh, W, cw, ch, p("loss"), p("record8"), s),
               ["loss", "record8"], 2 * n),
              ("crop_kl_loss_bwd", lambda L: L.art_flux_crop_kl_loss_bwd(p(flux), p(dims), p(truth), p("record8"), p(gl), B, Hh, W, cw, ch, p("grad_flux"),
                                                                         p("kl_ws"), s), ["grad_flux", "kl_ws"], 4 * n),
              ("center_of_mass", lambda L: L.art_flux_center_of_mass(p(flux), B, Hh, W, p("com"), s), ["com"], n),
              ("center_of_mass_bwd", lambda L: L.art_flux_center_of_mass_bwd(p("com"), p(gcomp), B, Hh, W, p("grad_flux"), s), ["grad_flux"], n)]
    return calls, buf


def run(fn, lib):
    code = fn(lib)
    if code != _lib.ART_OK:
        raise _lib.ArtistHipError(f"entry point returned {code}")


def time_variants(variants, B, rounds, steps):
    inp, cw, ch = metric_inputs(B)
    calls, _ = make_calls(inp, cw, ch)
    times = {(v, c[0]): [] for v, _ in variants for c in calls}
    st, en = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for rnd in range(rounds + 1):                       # (round 0 warms up)
        for name, fn, _, _ in calls:
            for vname, lib in variants:
                run(fn, lib)
                st.record()
                for _ in range(steps):
                    run(fn, lib)
                en.record()
                torch.cuda.synchronize()
                if rnd > 0:
                    times[(vname, name)].append(st.elapsed_time(en) / steps)
    out = {}
    for vname, _ in variants:
        out[vname] = {}
        for name, _, _, alg in calls:
            t = times[(vname, name)]
            med = statistics.median(t)
            out[vname][name] = {"ms": round(med, 4), "min_ms": round(min(t), 4), "max_ms": round(max(t), 4),
                                "algorithmic_GBps": round(alg / med / 1e6, 1),
                                "frac_of_8TBps": round(alg / med / 1e6 / 8000, 3)}
    return {"bitmaps": B, "resolution": [256, 256], "rounds": rounds, "steps": steps, "variants": out}


def compare_bits(variants):
    import flux_ref
    (na, la), (nb, lb) = variants
    os.environ["ARTIST_HIP_DEBUG"] = "1"                # (the library reads the parts knob only then)
    report, differing = [], 0
    shapes = [(flux_ref.case_id(c), lambda c=c: ({k: torch.from_numpy(v.copy()).to(DEV) for k, v in flux_ref.make_inputs(c).items()},
                                                  flux_ref.CROP_W, flux_ref.CROP_H)) for c in flux_ref.CASES]
    shapes.append(("metric-1000x256x256", lambda: metric_inputs(1000)))
    for shape, make in shapes:
        print(shape, file=sys.stderr, flush=True)
        inp, cw, ch = make()
        calls, buf = make_calls(inp, cw, ch)
        for parts in (None, "1", "2", "4"):
            os.environ.pop("ARTIST_HIP_LOSS_PARTS", None)
            if parts is not None:
                os.environ["ARTIST_HIP_LOSS_PARTS"] = parts
            for name, fn, outs, _ in calls:         # (a later call reads the records library B left: equal ones if all is well)
                if parts is not None and not name.startswith("crop_pixel_loss"):
                    continue
                if _lib.ART_EINVAL in [fn(lib) for lib in (la, lb)]:     # a loss kind that an older build does not know
                    report.append({"case": shape, "parts": parts or "unset", "call": name, "buffer": None, "verdict": "not in both libraries"})
                    continue
                got = []
                for lib in (la, lb):
                    for o in outs:
                        buf[o].fill_(float("nan"))
                    run(fn, lib)
                    got.append({o: buf[o].clone() for o in outs})
                for o in outs:
                    equal = bool(torch.equal(got[0][o].view(torch.int32), got[1][o].view(torch.int32)))
                    differing += not equal
                    report.append({"case": shape, "parts": parts or "unset", "call": name, "buffer": o, "verdict": "equal" if equal else "DIFFERENT"})
    os.environ.pop("ARTIST_HIP_LOSS_PARTS", None)
    return {"libraries": [na, nb], "comparisons": len(report), "different": differing, "report": report}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--bits", action="store_true")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--out")
    ap.add_argument("args", nargs="*", help="bitmap counts and NAME=path/to/lib.so variants")
    args = ap.parse_intermixed_args()
    sizes = [int(a) for a in args.args if "=" not in a] or [1000]
    variants = []
    for spec in [a for a in args.args if "=" in a] or ["lib="]:
        name, _, path = spec.partition("=")
        variants.append((name, _lib.bind(ctypes.CDLL(str(pathlib.Path(path).resolve())), path) if path else _lib.lib()))
    if args.bits:
        if len(variants) != 2:
            ap.error("--bits takes two NAME=path libraries")
        results = [compare_bits(variants)]
        print(f"{results[0]['comparisons']} comparisons, {results[0]['different']} different")
        for r in results[0]["report"]:
            if r["verdict"] != "equal":
                print(r)
    else:
        results = [time_variants(variants, B, args.rounds, args.steps) for B in sizes]
        for r in results:
            print(json.dumps(r))
    if args.out:
        pathlib.Path(args.out).write_text("".join(json.dumps(r) + "\n" for r in results))
    return 3 if args.bits and results[0]["different"] else 0           # (1: an exception)


if __name__ == "__main__":
    sys.exit(main())
