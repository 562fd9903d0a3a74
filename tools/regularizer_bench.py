#!/usr/bin/env python3
"""Cost of the surface regularisers -> profiles/regularizer_bench.json.

For the metric field (1000 heliostats x 4 facets x 10 x 10 control points) and one rank's share of it (125 heliostats):
  * HIP: art_surface_regularizers_fwd + _bwd through artist_amd.regularizers (both terms, per net, then the gradient w.r.t. the
    control points for given upstream gradients), device-event time per forward + backward;
  * torch: the same math as eager torch on the GPU - the reference's recipe (artist/optim/regularizers.py:116-131, 176-186),
    restated here - forward + autograd backward, the same way;
  * kernel launches per forward + backward of each (torch.profiler, in a pass of its own), the algorithmic bytes of the HIP
    pair (each input read once per pass, each output written once), and how far the two results are apart.

usage: python tools/regularizer_bench.py [--steps 200 --warmup 20] [--out FILE]
"""
import argparse
import json
import pathlib
import sys

import torch

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

SIZES = {"metric_field": (1000, 4, 10, 10), "rank_share_125": (125, 4, 10, 10)}


def torch_terms(current, original):
    """The reference's two regularisers before their reduction, eager torch (restated)."""
    delta = current - original
    padded = torch.nn.functional.pad(delta, (0, 0, 1, 1, 1, 1), mode="replicate")
    laplace = (4 * delta - padded[:, :, :-2, 1:-1, :] - padded[:, :, 2:, 1:-1, :] - padded[:, :, 1:-1, :-2, :]
               - padded[:, :, 1:-1, 2:, :])
    return (laplace ** 2).mean(dim=(2, 3, 4)), (delta ** 2).mean(dim=(2, 3, 4))


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


def launches(fn):
    """Device kernels per call of ``fn`` (torch.profiler; None where it records no device activity)."""
    from torch.profiler import ProfilerActivity, profile
    fn()
    torch.cuda.synchronize()
    try:
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
    except RuntimeError as exc:                       # (a profiler that cannot start: the timings still stand)
        return {"error": str(exc)[:200]}
    names = [e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]
    kernels = [nm for nm in names if not nm.lower().startswith(("memcpy", "memset"))]
    return {"kernels": len(kernels), "names": sorted(set(kernels))} if names else None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "regularizer_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("regularizer_bench needs a GPU")
    from artist_amd.regularizers import surface_regularizers

    dev = torch.device("cuda:0")
    result = {"device": torch.cuda.get_device_name(dev), "torch": torch.__version__, "steps": args.steps, "warmup": args.warmup,
              "timing": "device events around forward + backward, median over steps", "sizes": {}}
    for label, (H, F, U, V) in SIZES.items():
        g = torch.Generator().manual_seed(3)
        org = torch.randn(H, F, U, V, 3, generator=g)
        cur = (org + 2e-5 * torch.randn(H, F, U, V, 3, generator=g)).to(dev).requires_grad_(True)
        org = org.to(dev)
        up_s, up_i = torch.rand(H, F, device=dev), torch.rand(H, F, device=dev)

        def hip_step():
            s, i = surface_regularizers(cur, org)
            return torch.autograd.grad((s, i), cur, grad_outputs=(up_s, up_i))[0]

        def torch_step():
            s, i = torch_terms(cur, org)
            return torch.autograd.grad((s, i), cur, grad_outputs=(up_s, up_i))[0]

        s_h, i_h = surface_regularizers(cur, org)
        s_t, i_t = torch_terms(cur, org)
        g_h, g_t = hip_step(), torch_step()
        rel = lambda a, b: float((a - b).norm() / b.norm())  # noqa: E731
        n = U * V * 3
        N = H * F
        bytes_fwd = 2 * N * n * 4 + 2 * N * 4                     # current + original in, both terms out
        bytes_bwd = 2 * N * n * 4 + 2 * N * 4 + N * n * 4          # current + original + upstream in, gradient out
        hip = event_ms(hip_step, args.steps, args.warmup)
        tch = event_ms(torch_step, args.steps, args.warmup)
        entry = {
            "shape": [H, F, U, V, 3],
            "hip_fwd_bwd": hip, "torch_fwd_bwd": tch,
            "speedup_median": tch["median_ms"] / hip["median_ms"],
            "hip_launches": launches(hip_step), "torch_launches": launches(torch_step),
            "algorithmic_bytes": {"fwd": bytes_fwd, "bwd": bytes_bwd, "total": bytes_fwd + bytes_bwd},
            "hip_effective_GBps": (bytes_fwd + bytes_bwd) / (hip["median_ms"] * 1e-3) / 1e9,
            "hip_vs_torch_rel_l2": {"smoothness": rel(s_h, s_t), "ideal": rel(i_h, i_t), "gradient": rel(g_h, g_t)},
        }
        result["sizes"][label] = entry
        print(f"{label}: HIP fwd+bwd {hip['median_ms'] * 1e3:.1f} us, torch {tch['median_ms'] * 1e3:.1f} us "
              f"({entry['speedup_median']:.1f}x), launches {entry['hip_launches']} vs "
              f"{(entry['torch_launches'] or {}).get('kernels')}, {entry['hip_effective_GBps']:.0f} GB/s algorithmic", flush=True)
    out = pathlib.Path(args.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(json.dumps(result, indent=1) + "\n")
    print(f"wrote {out}")


if __name__ == "__main__":
    main()
