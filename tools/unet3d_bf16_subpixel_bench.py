"""A/B of `bf16_subpixel: true` against its parent mode `compute_dtype: bf16` on a UNet3D, both arms in ONE process and alternating,
as tools/unet2d_bench.py does for the 2-D keys: the chip is warmed past its ramp steps first, then every repeat times `--steps`
training steps of the parent arm and of the new arm back to back, so clock and thermal drift hit both alike.

    python tools/unet3d_bf16_subpixel_bench.py --patch 64,128,128 --batch 2          # the headline shape (3 of 3 levels eligible)
    python tools/unet3d_bf16_subpixel_bench.py --patch 80,170,170 --batch 1          # the shipped patch (2 of 3)

Prints one JSON line: per arm the per-repeat step times, their median and spread (max - min) and the peak memory of a step, then the
HIP-event time per step of every entry point of the decoders' first convolutions in each arm, summed per entry point and split per layer by
the FLOPs a launch declares (a pass of its own: the event packets cost device time)."""
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

NEW = ("u3d_subpixel_conv_fwd_bf16", "u3d_subpixel_conv_dgrad_bf16", "u3d_subpixel_conv_wgrad_bf16", "u3d_conv3d_wgrad_bf16_strided",
       "u3d_pack_subpixel_weights_bf16", "u3d_pack_weights_bf16_slice")
OLD = ("u3d_nearest_cat_fwd", "u3d_conv3d_bf16_ex", "u3d_conv3d_wgrad_bf16_job", "u3d_gn_bwd_apply_up", "u3d_gn_bwd_apply",
       "u3d_gn_bwd_finalize_split", "u3d_pack_weights_bf16_batch")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--f-maps", type=int, default=32)
    ap.add_argument("--levels", type=int, default=4)
    ap.add_argument("--patch", default="64,128,128")
    ap.add_argument("--batch", type=int, default=2)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=4)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    D, H, W = (int(v) for v in args.patch.split(","))
    torch.manual_seed(0)
    x = torch.randn(args.batch, 1, D, H, W, device=dev)
    target = (torch.rand(args.batch, 1, D, H, W, device=dev) > 0.5).float()
    crit = BCEDiceLoss()
    arms = {}
    for name, extra in (("bf16", dict(compute_dtype="bf16")), ("bf16_subpixel", dict(bf16_subpixel=True))):
        torch.manual_seed(1)
        arms[name] = get_model(dict(name="UNet3D", in_channels=1, out_channels=1, f_maps=args.f_maps, num_levels=args.levels,
                                    layer_order="gcr", num_groups=8, final_sigmoid=True, **extra)).to(dev).train()
        assert arms[name].native_supported, arms[name]._native_blockers

    def step(model):
        model.zero_grad(set_to_none=True)
        _, logits = model(x, return_logits=True)
        crit(logits, target).backward()

    eligible = len(arms["bf16_subpixel"]._get_engine()._subpixel_layers((D, H, W)).bf16_ids)
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
    fams, layers = {}, {}
    for name, model in arms.items():
        prof = nat.EventProfiler(only=NEW + OLD)
        nat.profiler = prof
        for _ in range(args.steps):
            step(model)
        torch.cuda.synchronize()
        nat.profiler = None
        fams[name] = {k: {"calls_per_step": v["calls"] / args.steps, "ms_per_step": round(v["ms"] / args.steps, 3)}
                      for k, v in sorted(prof.summary().items(), key=lambda kv: -kv[1]["ms"])}
        # ... and split per layer: a launch declares its FLOPs, and the decoders' first convolutions (whole, skip half, upsampled half) are
        # the only launches of their entry points with theirs; position = order within the step (u3d_conv3d_bf16_ex: forward, then data gradient)
        calls = {}
        for k, flops, st, en in prof.records:
            calls.setdefault((k, round(flops / 1e9, 2)), []).append(st.elapsed_time(en))
        layers[name] = {f"{k} {g} GFLOP": [round(sum(ms[i::len(ms) // args.steps]) / args.steps, 3) for i in range(len(ms) // args.steps)]
                        for (k, g), ms in sorted(calls.items(), key=lambda kv: (kv[0][0], -kv[0][1])) if g > 0 and len(ms) % args.steps == 0}
    out = {"model": "UNet3D", "f_maps": args.f_maps, "levels": args.levels, "patch": [D, H, W], "batch": args.batch,
           "eligible_levels": eligible, "decoders": args.levels - 1, "steps_per_repeat": args.steps, "repeats": args.repeats}
    for name in arms:
        t = times[name]
        out[name] = {"ms_per_step": [round(v, 2) for v in t], "median_ms": round(statistics.median(t), 2),
                     "spread_ms": round(max(t) - min(t), 2), "peak_mem_gb": round(peak[name] / 2**30, 3), "entry_points": fams[name],
                     "per_layer_ms": layers[name]}
    a, b = out["bf16"]["median_ms"], out["bf16_subpixel"]["median_ms"]
    out["speedup"] = round(a / b, 4)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
