"""Which entry points one training step launches, in order, with the FLOPs each call declares — held against the sequence the commit
before the `native_2d*` keys were resolved from one table launched on the MI355X (tests/golden/launch_sequences_2d.json).  Equality: the
kernel families are chosen on the host, and a call's declared FLOPs encode its channel counts and grid, so a layer routed to another
family or with the wrong half-widths shows up.

The cases are the smallest shapes of the model tests at which each routing rule has both outcomes; two 3-D models stand in for the
executor code the 2-D path shares.

`python tests/test_gpu_launch_sequence_2d.py record [path]` records the fixture: one child process per case under its own time limit,
stopping at the first that fails."""
import json
import os
import subprocess
import sys

import pytest

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "launch_sequences_2d.json")
CASES = {  # name: (class, model keys, f_maps, num_groups, input shape)
    "unet2d": ("UNet2D", dict(native_2d=True), [8, 16, 32], 4, (2, 1, 34, 40)),  # one exact-2x level, one n -> 2n + 1
    "unet2d_subpixel": ("UNet2D", dict(native_2d=True, native_2d_subpixel=True), [8, 16, 32], 4, (2, 1, 34, 40)),
    "unet2d_stem": ("UNet2D", dict(native_2d_stem=True), [8, 16], 4, (2, 1, 35, 45)),  # the second layer falls through for its data gradient
    "unet2d_bf16": ("UNet2D", dict(native_2d_bf16=True), [32, 64, 128], 8, (2, 1, 35, 45)),
    "unet2d_bf16_stem": ("UNet2D", dict(native_2d_bf16=True, native_2d_stem=True), [16, 32], 8, (2, 1, 35, 45)),  # `_c16` entry points
    "unet2d_bf16_vcat": ("UNet2D", dict(native_2d_bf16_vcat=True), [32, 64, 128], 8, (2, 1, 35, 45)),  # `_src` entry points
    # halves outside the `_src` envelope: the written-out concat
    "unet2d_bf16_vcat_stem": ("UNet2D", dict(native_2d_bf16_vcat=True, native_2d_stem=True), [16, 32], 8, (2, 1, 35, 45)),
    "resunet2d": ("ResidualUNet2D", dict(native_2d_residual=True), [8, 16, 32], 4, (2, 1, 35, 29)),
    "resunet2d_bf16": ("ResidualUNet2D", dict(native_2d_residual_bf16=True), [32, 64], 8, (2, 1, 32, 32)),
    "resunet2d_bf16_deconv": ("ResidualUNet2D", dict(native_2d_residual_bf16_deconv=True), [32, 64], 8, (2, 1, 32, 32)),
    "unet3d": ("UNet3D", dict(), [8, 16], 4, (1, 1, 9, 16, 16)),  # a plus level
    "resunet3d_bf16": ("ResidualUNet3D", dict(compute_dtype="bf16"), [32, 64], 8, (1, 1, 8, 16, 16)),
}


class _Recorder:
    """what `_native.profiler` needs: wrap(name, fn, args, flops); no events"""

    def __init__(self):
        self.calls = []

    def wrap(self, name, fn, args, flops):
        self.calls.append([name, float(flops)])
        return fn(*args)


def launch_sequence(case, cases=CASES):
    """[[entry point, declared FLOPs], ...] of one training forward + backward"""
    import torch

    from pytorch3dunet_amd import _native as nat
    from pytorch3dunet_amd.unet3d.model import get_model

    name, keys, f_maps, groups, shape = cases[case]
    torch.manual_seed(0)
    model = get_model(dict(name=name, in_channels=1, out_channels=1, f_maps=f_maps, num_groups=groups, **keys))
    assert model.native_supported, model._native_blockers
    dev = torch.device("cuda", 0)
    model = model.to(dev).train()
    x = torch.randn(shape).to(dev)
    rec = _Recorder()
    nat.profiler = rec
    try:
        _, logits = model(x, return_logits=True)
        (logits * logits).mean().backward()
        torch.cuda.synchronize()
    finally:
        nat.profiler = None
    return rec.calls


@pytest.mark.gpu
@pytest.mark.parametrize("case", list(CASES))
def test_launch_sequence(case):
    with open(FIXTURE) as fh:
        want = json.load(fh)[case]
    got = launch_sequence(case)
    assert len(got) > 0
    diff = next((i for i, (a, b) in enumerate(zip(got, want)) if a != b), min(len(got), len(want)))
    assert got == want, f"{len(got)} launches against {len(want)}; first difference at {diff}: {got[diff:diff + 2]} / {want[diff:diff + 2]}"


def record(path):
    out = {}
    for case in CASES:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "case", case], capture_output=True, text=True, timeout=180)
        if r.returncode != 0:
            sys.exit(f"{case}: exit status {r.returncode}; nothing further is run\n{r.stderr[-3000:]}")
        out[case] = json.loads(r.stdout.strip().splitlines()[-1])
        print(f"{case}: {len(out[case])} launches", flush=True)
    with open(path, "w") as fh:
        json.dump(out, fh, separators=(",", ":"))
        fh.write("\n")


if __name__ == "__main__":
    _root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.join(_root, "pytorch-3dunet_amd"))
    if sys.argv[1] == "case":
        print(json.dumps(launch_sequence(sys.argv[2])))
    else:
        assert sys.argv[1] == "record", sys.argv
        record(sys.argv[2] if len(sys.argv) > 2 else FIXTURE)
