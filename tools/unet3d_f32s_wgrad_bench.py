"""A/B of `fp32_split_wgrad: true` against its parent mode `compute_dtype: fp32_split`, both arms in ONE process and alternating, as
tools/unet3d_bf16_stem_bench.py does for its key: the chip is warmed past its ramp steps first, then every repeat times `--steps`
training steps of the parent arm and of the new arm back to back, so clock and thermal drift hit both alike.

    python tools/unet3d_f32s_wgrad_bench.py --patch 64,128,128 --batch 2                                  # the headline shape
    python tools/unet3d_f32s_wgrad_bench.py --patch 80,170,170 --batch 1                                  # the shipped patch
    python tools/unet3d_f32s_wgrad_bench.py --model ResidualUNet3D --f-maps 64 --levels 5 --patch 80,160,160 --batch 1   # config 4's net

Prints one JSON line: per arm the per-repeat step times, their median and range, whether the two ranges are disjoint and the peak memory
of a step; then, from a pass of its own (the event packets cost device time), the HIP-event time per step of the entry points that differ
between the arms, and per routed layer the u3d_conv3d_wgrad_f32s launch next to the u3d_conv3d_wgrad_job launch it replaces (the weight
gradient launches of a step come in the same order in both arms; the job launch also carries the GroupNorm-backward reduction, which the
new arm runs as u3d_gn_bwd_finalize* launches of their own — listed under `entry_points`)."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "pytorch-3dunet_amd"))
import torch  # noqa: E402

from pytorch3dunet_amd import _native as nat  # noqa: E402
from pytorch3dunet_amd.unet3d.losses import BCEDiceLoss  # noqa: E402
from pytorch3dunet_amd.unet3d.model import get_model  # noqa: E402

NEW = "u3d_conv3d_wgrad_f32s"
OLD = "u3d_conv3d_wgrad_job"
SIDE = ("u3d_gn_bwd_finalize", "u3d_gn_bwd_finalize_split")
PEAK_BF16 = 2500.0  # dense TFLOP/s, MI355X_MICROARCH.md


class _Prof(nat.EventProfiler):
    """... that also keeps (N, D, H, W, Cin, Cout) of every new launch"""

    def __init__(self, **kw):
        super().__init__(**kw)
        self.shapes = []

    def wrap(self, name, fn, args, flops):
        n0 = len(self.records)
        rc = super().wrap(name, fn, args, flops)
        if len(self.records) > n0:
            self.shapes.append(tuple(args[7:13]) if name == NEW else None)
        return rc


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="UNet3D")
    ap.add_argument("--f-maps", default="32", help="an integer, or a comma-separated list of per-level widths")
    ap.add_argument("--levels", type=int, default=4)
    ap.add_argument("--patch", default="64,128,128")
    ap.add_argument("--batch", type=int, default=2)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=4)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    D, H, W = (int(v) for v in args.patch.split(","))
    f_maps = [int(v) for v in args.f_maps.split(",")] if "," in args.f_maps else int(args.f_maps)
    torch.manual_seed(0)
    x = torch.randn(args.batch, 1, D, H, W, device=dev)
    target = (torch.rand(args.batch, 1, D, H, W, device=dev) > 0.5).float()
    crit = BCEDiceLoss()
    arms = {}
    for name, extra in (("fp32_split", dict(compute_dtype="fp32_split")), ("fp32_split_wgrad", dict(fp32_split_wgrad=True))):
        torch.manual_seed(1)
        arms[name] = get_model(dict(name=args.model, in_channels=1, out_channels=1, f_maps=f_maps, num_levels=args.levels,
                                    layer_order="gcr", num_groups=8, final_sigmoid=True, **extra)).to(dev).train()
        assert arms[name].native_supported, arms[name]._native_blockers

    def step(model):
        model.zero_grad(set_to_none=True)
        _, logits = model(x, return_logits=True)
        crit(logits, target).backward()

    for _ in range(args.warmup):  # past the chip's ramp steps, both arms
        for model in arms.values():
            step(model)
    torch.cuda.synchronize()
    times = {k: [] for k in arms}
    peak = {}
    for _ in range(args.repeats):
        for name, model in arms.items():
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                step(model)
            torch.cuda.synchronize()
            times[name].append((time.perf_counter() - t0) / args.steps * 1e3)
            peak[name] = max(peak.get(name, 0), torch.cuda.max_memory_allocated())
    fams, seq = {}, {}
    for name, model in arms.items():
        prof = _Prof(only=(NEW, OLD) + SIDE)
        nat.profiler = prof
        for _ in range(args.steps):
            step(model)
        torch.cuda.synchronize()
        nat.profiler = None
        fams[name] = {k: {"calls_per_step": v["calls"] / args.steps, "ms_per_step": round(v["ms"] / args.steps, 3)}
                      for k, v in sorted(prof.summary().items(), key=lambda kv: -kv[1]["ms"])}
        # the weight-gradient launches of a step, in order: [(entry point, GFLOP, ms averaged over the steps, shape)]
        rows = [(k, flops, st.elapsed_time(en), sh) for (k, flops, st, en), sh in zip(prof.records, prof.shapes) if k in (NEW, OLD)]
        per = len(rows) // args.steps
        assert per * args.steps == len(rows)
        seq[name] = [(rows[i][0], rows[i][1], sum(r[2] for r in rows[i::per]) / args.steps, rows[i][3]) for i in range(per)]
    assert len(seq["fp32_split"]) == len(seq["fp32_split_wgrad"]), "the arms issue their weight gradients in the same order"
    layers = []
    for (k0, f0, ms0, _), (k1, f1, ms1, sh) in zip(seq["fp32_split"], seq["fp32_split_wgrad"]):
        assert k0 == OLD and abs(f0 - f1) <= 1e-9 * f0
        if k1 == NEW:
            layers.append({"N_D_H_W_Cin_Cout": list(sh), "gflop": round(f1 / 1e9, 2), "wgrad_job_ms": round(ms0, 3), "wgrad_f32s_ms": round(ms1, 3),
                           "ratio": round(ms0 / ms1, 3), "f32s_tflops_fp32_equivalent": round(f1 / ms1 / 1e9, 1),
                           "f32s_share_of_bf16_peak_executed": round(6 * f1 / ms1 / 1e9 / PEAK_BF16, 3)})
    out = {"model": args.model, "f_maps": f_maps, "levels": args.levels, "patch": [D, H, W], "batch": args.batch,
           "launches_on_the_new_kernel": len(layers), "steps_per_repeat": args.steps, "repeats": args.repeats}
    for name in arms:
        t = times[name]
        out[name] = {"ms_per_step": [round(v, 2) for v in t], "median_ms": round(statistics.median(t), 2), "min_ms": round(min(t), 2),
                     "max_ms": round(max(t), 2), "spread_ms": round(max(t) - min(t), 2), "peak_mem_gb": round(peak[name] / 2**30, 3),
                     "entry_points": fams[name]}
    a, b = out["fp32_split"]["median_ms"], out["fp32_split_wgrad"]["median_ms"]
    out["speedup"] = round(a / b, 4)
    out["ranges_disjoint"] = bool(max(times["fp32_split_wgrad"]) < min(times["fp32_split"]) or max(times["fp32_split"]) < min(times["fp32_split_wgrad"]))
    out["routed_layers"] = layers
    out["routed_sum_ms"] = {"wgrad_job": round(sum(r["wgrad_job_ms"] for r in layers), 3), "wgrad_f32s": round(sum(r["wgrad_f32s_ms"] for r in layers), 3)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
