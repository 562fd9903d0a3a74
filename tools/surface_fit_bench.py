#!/usr/bin/env python3
"""Cost of fitting NURBS control nets to measured normals -> profiles/surface_fit_bench.json.

For B in {4, 400, 4000} facets of N = 800 points, 10 x 10 control points of degree 3, 401 epochs (max_epoch = 400), normals
method, in the same process:
  (a) host loop: the best route without the fit kernels - artist_amd.NURBSSurfaces (scattered scheme, all facets batched in H) +
      torch.nn.functional.mse_loss + artist_amd.optim.Adam, one epoch = forward, loss, backward, step; no host read of the loss;
  (b) SurfaceGenerator.fit_nurbs_batch: one prepare launch + one run launch.
Wall time per complete fit between device synchronisations (a fit is tens to thousands of milliseconds: launch overhead is part
of what is measured), two warm-up fits first, median / min / max and the relative spread over the repetitions; and how far the
two results are apart.

With --points N the facets have N points each instead of 800 - above about 5000 `fit_nurbs_batch` evaluates a facet in chunks
 -; profiles/surface_fit_bench_large.json holds such runs, one entry per (N, B).

usage: python tools/surface_fit_bench.py [--reps 9 --loop-reps 5 --warmup 2 --sizes 4,400,4000] [--points N] [--out FILE]
"""
import argparse
import json
import pathlib
import sys
import time

import numpy as np
import torch

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

N, NET, DEG, MAX_EPOCH = 800, 10, 3, 400


def wall_ms(fn, reps, warmup=1):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    ms.sort()
    return {"median_ms": ms[len(ms) // 2], "min_ms": ms[0], "max_ms": ms[-1], "reps": reps, "warmup": warmup,
            "spread_rel": (ms[-1] - ms[0]) / ms[len(ms) // 2]}


def main():
    global N
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--loop-reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--sizes", default="4,400,4000")
    ap.add_argument("--points", type=int, default=N, help="points per facet (default 800)")
    ap.add_argument("--out", default=None, help="default: profiles/surface_fit_bench.json, or, with --points, "
                                                "profiles/surface_fit_bench_large.json, which gathers its runs under 'points'")
    args = ap.parse_args()
    large = args.points != N
    if args.out is None:
        args.out = str(ROOT / "profiles" / ("surface_fit_bench_large.json" if large else "surface_fit_bench.json"))
    N = args.points
    if not torch.cuda.is_available():
        raise SystemExit("surface_fit_bench needs a GPU")
    import surface_fit_ref as sfr
    from artist_amd import NURBSSurfaces, SurfaceGenerator, optim

    dev = torch.device("cuda:0")
    gen = SurfaceGenerator(torch.tensor([NET, NET]), torch.tensor([DEG, DEG]))
    base = [sfr.synthetic_facet(N, 2000 + k) for k in range(16)]
    result = {"device": torch.cuda.get_device_name(dev), "torch": torch.__version__, "points_per_facet": N, "net": [NET, NET],
              "degrees": [DEG, DEG], "epochs": MAX_EPOCH + 1, "method": "deflectometry (normals)",
              "timing": "wall time of a complete fit between device synchronisations, warm-up fits first, median over reps", "warmup": args.warmup, "sizes": {}}
    for B in [int(s) for s in args.sizes.split(",")]:
        pts = torch.from_numpy(np.stack([base[b % 16][0] for b in range(B)])).to(dev)
        nrm = torch.from_numpy(np.stack([base[b % 16][1] for b in range(B)])).to(dev)
        prep = gen.prepare(pts)
        uv, cp0 = prep.eval_uv.reshape(B, 1, N, 2), prep.initial_control_points.reshape(B, 1, NET, NET, 3)
        target = nrm.reshape(B, 1, N, 4)
        out = {}

        def host_loop():
            cp = cp0.clone().requires_grad_(True)
            opt = optim.Adam([cp], lr=1e-3)
            surf = NURBSSurfaces(gen.degrees, cp, device=dev)        # built once per fit: the epochs launch nothing for it
            for _ in range(MAX_EPOCH + 1):
                _, normals = surf.calculate_surface_points_and_normals(uv, None, None)
                opt.zero_grad()
                loss = torch.nn.functional.mse_loss(normals, target, reduction="sum") / (N * 4)      # = sum of the facets' means
                loss.backward()
                opt.step()
            out["loop"] = cp.detach()

        def fused():
            out["fused"] = gen.fit_nurbs_batch(pts, nrm, fit_method="deflectometry", max_epoch=MAX_EPOCH)[0].control_points.detach()

        fused_t = wall_ms(fused, args.reps, args.warmup)
        loop_t = wall_ms(host_loop, args.loop_reps, args.warmup)
        diff = float((out["fused"].reshape(B, -1) - out["loop"].reshape(B, -1)).abs().max())
        entry = {"facets": B, "host_loop": loop_t, "fit_nurbs_batch": fused_t,
                 "speedup_median": loop_t["median_ms"] / fused_t["median_ms"],
                 "fused_us_per_facet_epoch": fused_t["median_ms"] * 1e3 / (B * (MAX_EPOCH + 1)),
                 "max_abs_control_point_difference": diff}
        result["sizes"][str(B)] = entry
        print(f"B={B}: host loop {loop_t['median_ms']:.1f} ms, fit_nurbs_batch {fused_t['median_ms']:.1f} ms "
              f"({entry['speedup_median']:.1f}x), max |cp difference| {diff:.2e}", flush=True)
        out_path = pathlib.Path(args.out)
        out_path.parent.mkdir(parents=True, exist_ok=True)
        doc = result
        if large:       # one file for all point counts: this run's entry beside the ones already there
            doc = json.loads(out_path.read_text()) if out_path.exists() else {"points": {}}
            doc["points"].setdefault(str(N), result)["sizes"].update(result["sizes"])
        out_path.write_text(json.dumps(doc, indent=1) + "\n")
    print(f"wrote {args.out}")


if __name__ == "__main__":
    main()
