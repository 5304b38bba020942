"""A/B of `bf16_stem: true` against its parent mode `compute_dtype: bf16` on a UNet3D, both arms in ONE process and alternating, as
tools/unet3d_bf16_subpixel_bench.py does for its key: the chip is warmed past its ramp steps first, then every repeat times `--steps`
training steps of the parent arm and of the new arm back to back, so clock and thermal drift hit both alike.

    python tools/unet3d_bf16_stem_bench.py --patch 64,128,128 --batch 2 --repeats 15              # the headline shape: encoders.0's 16 -> 32
    python tools/unet3d_bf16_stem_bench.py --patch 80,170,170 --batch 1 --repeats 15              # the shipped patch
    python tools/unet3d_bf16_stem_bench.py --f-maps 16,32,64,128,256 --patch 128,128,128 --batch 1 --repeats 15   # the denoising net

Prints one JSON line: per arm the per-repeat step times, their median and spread (max - min), whether the two ranges are disjoint and the
peak memory of a step; then the HIP-event time per step of the entry points that differ between the arms (a pass of its own: the event
packets cost device time), summed per entry point and split per layer by the FLOPs a launch declares; and for the full-resolution
16 -> 32 layer of `encoders.0` (`f_maps: 32`) each new launch next to the fp32 launch it replaces, with its rate on the bytes it must move
(forward: x + out; data gradient: dz + gx + dg; weight gradient: x + dz)."""
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

NEW = ("u3d_conv3d_bf16_c16", "u3d_conv3d_wgrad_bf16_c16", "u3d_pack_weights_bf16_c16")
OLD = ("u3d_conv3d_ex_reps", "u3d_conv3d_wgrad_job", "u3d_nearest_cat_fwd", "u3d_subpixel_conv_fwd", "u3d_subpixel_conv_dgrad_reps",
       "u3d_subpixel_conv_wgrad", "u3d_gn_bwd_finalize", "u3d_pack_weights_batch_cells", "u3d_pack_weights_batch")


def main():
    ap = argparse.ArgumentParser()
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
    for name, extra in (("bf16", dict(compute_dtype="bf16")), ("bf16_stem", dict(bf16_stem=True))):
        torch.manual_seed(1)
        arms[name] = get_model(dict(name="UNet3D", in_channels=1, out_channels=1, f_maps=f_maps, num_levels=args.levels,
                                    layer_order="gcr", num_groups=8, final_sigmoid=True, **extra)).to(dev).train()
        assert arms[name].native_supported, arms[name]._native_blockers

    def step(model):
        model.zero_grad(set_to_none=True)
        _, logits = model(x, return_logits=True)
        crit(logits, target).backward()

    routed = len(arms["bf16_stem"]._get_engine().images._each_bf16_c16)
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
        # ... and split per layer: a launch declares its FLOPs; position = order within the step (the conv entry points: forward, then
        # data gradient)
        calls = {}
        for k, flops, st, en in prof.records:
            calls.setdefault((k, round(flops / 1e9, 2)), []).append(st.elapsed_time(en))
        layers[name] = {f"{k} {g} GFLOP": [round(sum(ms[i::len(ms) // args.steps]) / args.steps, 3) for i in range(len(ms) // args.steps)]
                        for (k, g), ms in sorted(calls.items(), key=lambda kv: (kv[0][0], -kv[0][1])) if g > 0 and len(ms) % args.steps == 0}
    out = {"model": "UNet3D", "f_maps": f_maps, "levels": args.levels, "patch": [D, H, W], "batch": args.batch, "layers_on_new_kernels": routed,
           "steps_per_repeat": args.steps, "repeats": args.repeats}
    for name in arms:
        t = times[name]
        out[name] = {"ms_per_step": [round(v, 2) for v in t], "median_ms": round(statistics.median(t), 2), "min_ms": round(min(t), 2),
                     "max_ms": round(max(t), 2), "spread_ms": round(max(t) - min(t), 2), "peak_mem_gb": round(peak[name] / 2**30, 3),
                     "entry_points": fams[name], "per_layer_ms": layers[name]}
    a, b = out["bf16"]["median_ms"], out["bf16_stem"]["median_ms"]
    out["speedup"] = round(a / b, 4)
    out["ranges_disjoint"] = bool(max(times["bf16_stem"]) < min(times["bf16"]) or max(times["bf16"]) < min(times["bf16_stem"]))
    if f_maps == 32:
        # encoders.0's second convolution, 16 -> 32 at full resolution: the only launches with its FLOPs on the conv entry points
        V = args.batch * D * H * W
        g = round(54.0 * 16 * 32 * V / 1e9, 2)
        must = {"forward": V * (16 + 32) * 4, "data_gradient": V * (32 + 16 + 16) * 4, "weight_gradient": V * (16 + 32) * 4}
        old = (layers["bf16"].get(f"u3d_conv3d_ex_reps {g} GFLOP", []) + [None, None])[:2] + \
              (layers["bf16"].get(f"u3d_conv3d_wgrad_job {g} GFLOP", []) + [None])[:1]
        new = (layers["bf16_stem"].get(f"u3d_conv3d_bf16_c16 {g} GFLOP", []) + [None, None])[:2] + \
              (layers["bf16_stem"].get(f"u3d_conv3d_wgrad_bf16_c16 {g} GFLOP", []) + [None])[:1]
        out["encoders0_16_to_32"] = {
            d: {"fp32_ms": o, "bf16_c16_ms": n, "must_move_mb": round(nb / 1e6, 1),
                "bf16_c16_gb_per_s": round(nb / 1e9 / (n / 1e3), 1) if n else None}
            for d, o, n, nb in zip(must, old, new, must.values())}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
