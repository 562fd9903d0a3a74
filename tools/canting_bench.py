#!/usr/bin/env python3
"""Cost of the canting rotation on its own -> profiles/canting_bench.json.

For the metric field (1000 heliostats x 4 facets x 2500 points) and one rank's share of it (125 heliostats), each entry point
called through the binding on preallocated buffers, device events around every call, median over the steps:
  * art_cant_facets_fwd (points + translations and normals) against its traffic, 64 B per point (two float4 in, two out);
  * art_cant_facets_bwd with all four gradients against 96 B per point (data and upstream gradients in, data gradients out),
    and with the canting / translation gradients alone (64 B per point, nothing written but 48 B per facet);
  * the fused art_nurbs_fwd / art_nurbs_bwd with canting and translations (what a field whose canting does not learn
    launches), and the same two without them (stage one of the two-stage route): the price of the route is
    (stage one + canting) - fused, forward and backward.
The achieved rate is algorithmic bytes over the median time; DESIGN.md 4.0 holds the streaming rates of this machine class
(7.05 TB/s read, 5.5 TB/s copy) it is compared with.

usage: python tools/canting_bench.py [--steps 200 --warmup 20] [--out FILE]
"""
import argparse
import json
import pathlib
import sys

import torch

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

SIZES = {"rank_share_125": 125, "metric_field": 1000}
F, N_EVAL, N_CP, DEGREE = 4, 50, (10, 10), 3
COPY_TBPS, READ_TBPS = 5.50, 7.05                    # DESIGN.md 4.0 (tools/hbm_peak.hip)


def event_ms(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    pairs = []
    for _ in range(steps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        pairs.append((a, b))
    torch.cuda.synchronize()
    ms = sorted(a.elapsed_time(b) for a, b in pairs)
    return {"median_ms": ms[len(ms) // 2], "mean_ms": sum(ms) / len(ms), "min_ms": ms[0], "max_ms": ms[-1]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "canting_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("canting_bench needs a GPU")
    from artist_amd import NURBSSurfaces, _lib, create_nurbs_evaluation_grid
    from artist_amd.scene import synthetic_control_points

    dev = torch.device("cuda:0")
    result = {"device": torch.cuda.get_device_name(dev), "torch": torch.__version__, "steps": args.steps, "warmup": args.warmup,
              "timing": "device events around each call of the entry point, median over steps",
              "streaming_rates_TBps": {"copy": COPY_TBPS, "read": READ_TBPS, "source": "DESIGN.md 4.0"}, "sizes": {}}
    for label, H in SIZES.items():
        g = torch.Generator().manual_seed(3)
        cp, cant, tr = synthetic_control_points(H, N_CP, 1e-3, device=dev)
        cant = (cant + (3e-3 * torch.randn(cant.shape, generator=g)).to(dev) * torch.tensor([1.0, 1.0, 1.0, 0.0], device=dev)).contiguous()
        tr = tr.contiguous()
        surf = NURBSSurfaces(torch.tensor([DEGREE, DEGREE]), cp, device=dev)
        uv = create_nurbs_evaluation_grid(torch.tensor([N_EVAL, N_EVAL]), device=dev)[None, None].expand(H, F, -1, -1)
        M = N_EVAL * N_EVAL
        with torch.no_grad():
            p0, n0 = surf.calculate_surface_points_and_normals(uv, None, None)
        ku, kv = (k.expand(H, F, -1).contiguous() for k in (surf.knot_vectors_u, surf.knot_vectors_v))
        nu, nv = N_CP
        nuq = (nu - DEGREE + 1, nv - DEGREE + 1)
        new = lambda *shape: torch.empty(shape, dtype=torch.float32, device=dev)  # noqa: E731
        out_p, out_n, gd_p, gd_n, g_cp = new(H, F, M, 4), new(H, F, M, 4), new(H, F, M, 4), new(H, F, M, 4), torch.empty_like(cp)
        g_c, g_t = new(H, F, 2, 4), new(H, F, 4)
        up_p = (torch.rand(H, F, M, 4, generator=g) - 0.5).to(dev)
        up_n = (torch.rand(H, F, M, 4, generator=g) - 0.5).to(dev)
        P = lambda x: x.data_ptr()  # noqa: E731

        def nurbs_fwd(canted):
            _lib.call("art_nurbs_fwd", dev, P(cp), P(uv), uv.stride(0), uv.stride(1), P(ku), P(kv), P(cant) if canted else None,
                      P(tr) if canted else None, DEGREE, DEGREE, 1, nuq[0], nuq[1], H, F, M, nu, nv, None, P(out_p), P(out_n))

        def nurbs_bwd(canted):
            _lib.call("art_nurbs_bwd", dev, P(cp), P(uv), uv.stride(0), uv.stride(1), P(ku), P(kv), P(cant) if canted else None,
                      DEGREE, DEGREE, 1, nuq[0], nuq[1], H, F, M, nu, nv, None, P(up_p), P(up_n), P(g_cp))

        def cant_fwd():
            _lib.call("art_cant_facets_fwd", dev, P(cant), P(tr), P(p0), P(n0), 0, H * F, M, P(out_p), P(out_n))

        def cant_bwd(data_grads):
            _lib.call("art_cant_facets_bwd", dev, P(cant), P(p0), P(n0), P(up_p), P(up_n), 0, H * F, M,
                      P(gd_p) if data_grads else None, P(gd_n) if data_grads else None, P(g_c), P(g_t))

        legs = {
            "cant_facets_fwd": (cant_fwd, 64), "cant_facets_bwd": (lambda: cant_bwd(True), 96),
            "cant_facets_bwd_sums_only": (lambda: cant_bwd(False), 64),
            "nurbs_fwd_fused": (lambda: nurbs_fwd(True), None), "nurbs_fwd_uncanted": (lambda: nurbs_fwd(False), None),
            "nurbs_bwd_fused": (lambda: nurbs_bwd(True), None), "nurbs_bwd_uncanted": (lambda: nurbs_bwd(False), None),
        }
        entry = {"shape": [H, F, M, 4], "points": H * F * M}
        for name, (fn, bytes_per_point) in legs.items():
            timing = event_ms(fn, args.steps, args.warmup)
            if bytes_per_point is not None:
                nbytes = bytes_per_point * H * F * M
                rate = nbytes / (timing["median_ms"] * 1e-3) / 1e12
                timing.update(algorithmic_bytes=nbytes, bytes_per_point=bytes_per_point, achieved_TBps=rate,
                              share_of_copy_rate=rate / COPY_TBPS)
            entry[name] = timing
        med = lambda k: entry[k]["median_ms"]  # noqa: E731
        entry["two_stage_price_ms"] = {
            "fwd": med("nurbs_fwd_uncanted") + med("cant_facets_fwd") - med("nurbs_fwd_fused"),
            "bwd": med("nurbs_bwd_uncanted") + med("cant_facets_bwd") - med("nurbs_bwd_fused")}
        result["sizes"][label] = entry
        print(f"{label}: cant fwd {med('cant_facets_fwd') * 1e3:.1f} us ({entry['cant_facets_fwd']['achieved_TBps']:.2f} TB/s), "
              f"bwd {med('cant_facets_bwd') * 1e3:.1f} us ({entry['cant_facets_bwd']['achieved_TBps']:.2f} TB/s), sums only "
              f"{med('cant_facets_bwd_sums_only') * 1e3:.1f} us; nurbs fwd fused {med('nurbs_fwd_fused') * 1e3:.1f} / uncanted "
              f"{med('nurbs_fwd_uncanted') * 1e3:.1f} us, bwd fused {med('nurbs_bwd_fused') * 1e3:.1f} / uncanted "
              f"{med('nurbs_bwd_uncanted') * 1e3:.1f} us; two-stage price fwd {entry['two_stage_price_ms']['fwd'] * 1e3:.1f} us, "
              f"bwd {entry['two_stage_price_ms']['bwd'] * 1e3:.1f} us", flush=True)
    out = pathlib.Path(args.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(json.dumps(result, indent=1) + "\n")
    print(f"wrote {out}")


if __name__ == "__main__":
    main()
