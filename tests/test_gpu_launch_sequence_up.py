"""Which entry points one training step launches around the decoders' up-sampling, in order, with the FLOPs each call declares — held
against the sequence the commit before the up-sampling families were chosen from one table (`ConvLayers._up_family`, `_UP_KERNELS`)
launched on the MI355X (tests/golden/launch_sequences_up.json; recorded twice there, identical).  One case per family and per outcome of
the joining, each at the smallest shape that takes the branch; the recorder and the comparison are test_gpu_launch_sequence_2d.py's, whose
fixture already holds the `t8` family on fp32 storage (`resunet3d_bf16`), `convtr2d` (`resunet2d`) and `convtr2d_bf16`
(`resunet2d_bf16_deconv`).

`python tests/test_gpu_launch_sequence_up.py record [path]` records the fixture: one child process per case under its own time limit,
stopping at the first that fails or whose sequence lacks an entry point its row names."""
import json
import os
import subprocess
import sys

import pytest

from test_gpu_launch_sequence_2d import launch_sequence

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "launch_sequences_up.json")
_B16 = dict(compute_dtype="bf16", activation_dtype="bf16")
CASES = {  # name: (class, model keys, f_maps, num_groups, input shape)
    "unet3d_deconv": ("UNet3D", dict(upsample="deconv"), [8, 16], 4, (1, 1, 9, 16, 16)),  # nearest resize 7 x 15 x 15 -> 9 x 16 x 16
    # a channel count % 4 != 0.  (A DoubleConv net with upsample='deconv' needs f_maps that double, and its encoder's middle width 3 a
    # GroupNorm it divides: [6, 12] with 3 groups is the nearest such model to [6, 10] with 2)
    "unet3d_deconv_odd": ("UNet3D", dict(upsample="deconv"), [6, 12], 3, (1, 1, 9, 16, 16)),
    "unet3d_trilinear": ("UNet3D", dict(upsample="trilinear"), [8, 16], 4, (1, 1, 9, 16, 16)),
    "resunet3d": ("ResidualUNet3D", dict(), [8, 16, 32], 4, (1, 1, 9, 16, 16)),
    "resunet3d_odd": ("ResidualUNet3D", dict(), [6, 10], 2, (1, 1, 9, 16, 16)),
    "resunet3d_concat": ("ResidualUNet3D", dict(upsample="deconv"), [8, 16, 32], 4, (1, 1, 9, 16, 16)),
    # (bf16 storage needs blocks of channel counts % 64, `ResUNetEngine._act_bf16_blocker`: [64, 128] is the smallest such net)
    "resunet3d_b16": ("ResidualUNet3D", _B16, [64, 128], 8, (1, 1, 8, 16, 16)),
    # its low-res grid is test_gpu_b16.py's flat-tile case (5 x 10 x 10, 128 -> 64): u3d_convtr3d_fwd_t8_workspace_floats > 0
    "resunet3d_b16_splitk": ("ResidualUNet3D", _B16, [64, 128], 8, (1, 1, 10, 20, 20)),
    "resunet3d_ckpt": ("ResidualUNet3D", dict(checkpoint_encoders=True), [8, 16, 32], 4, (1, 1, 9, 16, 16)),  # lean tape, recomputation
    "resunet2d_concat": ("ResidualUNet2D", dict(native_2d_residual=True, upsample="deconv"), [8, 16], 4, (2, 1, 35, 29)),
}
REACHES = {  # entry points a case's sequence must contain (asserted when recording and by the test)
    "unet3d_deconv": ("u3d_convtr3d_fwd_subpixel", "u3d_convtr3d_bwd", "u3d_cvt_f64_f32"),
    "unet3d_deconv_odd": ("u3d_convtr3d_fwd", "u3d_convtr3d_bwd", "u3d_cvt_f64_f32"),
    "unet3d_trilinear": ("u3d_resample2_fwd", "u3d_resample2_bwd"),
    "resunet3d": ("u3d_convtr3d_fwd_subpixel", "u3d_nearest_add_fwd", "u3d_nearest_sum_bwd", "u3d_convtr3d_bwd"),
    "resunet3d_odd": ("u3d_convtr3d_fwd", "u3d_nearest_add_fwd", "u3d_nearest_sum_bwd", "u3d_convtr3d_bwd"),
    "resunet3d_concat": ("u3d_nearest_cat_fwd", "u3d_split_channels", "u3d_conv1x1_bwd", "u3d_convtr3d_bwd"),
    "resunet3d_b16": ("u3d_convtr3d_fwd_t8_b16", "u3d_nearest_add_fwd_t8_b16", "u3d_nearest_sum_bwd_t8_b16", "u3d_convtr3d_wgrad_t8_b16",
                      "u3d_convtr3d_dgrad_t8_b16_ex", "u3d_maxpool2_fwd_b16", "u3d_conv1x1_head_fwd_b16"),
    "resunet3d_b16_splitk": ("u3d_convtr3d_fwd_t8_b16_ex", "u3d_nearest_add_fwd_t8_b16", "u3d_convtr3d_dgrad_t8_b16_ex"),
    "resunet3d_ckpt": ("u3d_convtr3d_fwd_subpixel", "u3d_maxpool2_fwd", "u3d_maxpool2_bwd_merge"),
    "resunet2d_concat": ("u3d_convtr2d_fwd", "u3d_nearest_cat_fwd", "u3d_split_channels", "u3d_convtr2d_wgrad", "u3d_convtr2d_dgrad",
                         "u3d_maxpool2d_fwd"),
}
assert set(REACHES) == set(CASES)


def _missing(case, seq):
    names = {name for name, _ in seq}
    return [ep for ep in REACHES[case] if ep not in names]


@pytest.mark.gpu
@pytest.mark.parametrize("case", list(CASES))
def test_launch_sequence(case):
    with open(FIXTURE) as fh:
        want = json.load(fh)[case]
    got = launch_sequence(case, CASES)
    assert not _missing(case, got), _missing(case, got)
    diff = next((i for i, (a, b) in enumerate(zip(got, want)) if a != b), min(len(got), len(want)))
    assert got == want, f"{len(got)} launches against {len(want)}; first difference at {diff}: {got[diff:diff + 2]} / {want[diff:diff + 2]}"


def record(path):
    out = {}
    for case in CASES:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "case", case], capture_output=True, text=True, timeout=180)
        if r.returncode != 0:
            sys.exit(f"{case}: exit status {r.returncode}; nothing further is run\n{r.stderr[-3000:]}")
        out[case] = json.loads(r.stdout.strip().splitlines()[-1])
        if _missing(case, out[case]):
            sys.exit(f"{case}: the sequence does not reach {_missing(case, out[case])}; nothing further is run")
        print(f"{case}: {len(out[case])} launches", flush=True)
    with open(path, "w") as fh:
        json.dump(out, fh, separators=(",", ":"))
        fh.write("\n")


if __name__ == "__main__":
    _root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.join(_root, "pytorch-3dunet_amd"))
    if sys.argv[1] == "case":
        print(json.dumps(launch_sequence(sys.argv[2], CASES)))
    else:
        assert sys.argv[1] == "record", sys.argv
        record(sys.argv[2] if len(sys.argv) > 2 else FIXTURE)
