"""Which entry points one training step launches around the 3x3(x3) convolutions, in order, with the FLOPs each call declares — held
against the sequence the commit before a layer's kernel family was recorded once (`ConvRec.family`, `ConvLayers._bwd_families`) launched
on the MI355X (tests/golden/launch_sequences_conv.json; recorded twice there, identical; the two `unet2d_bf16_subpixel*` cases likewise at
the commit before `subpixel2d_bf16` became a recorded family of its own and a decoder's join one decision).  The cases are the conv-family outcomes the two
older fixtures do not reach, each at about the smallest shape that takes the branch; the recorder and the comparison are
test_gpu_launch_sequence_2d.py's.  (That recorder asks for no input gradient, so a stem layer on the bf16 kernels whose small-family
first layer needs a data gradient has no case here; `unet2d_stem` of the older fixture holds the small family's fall-through.)

`python tests/test_gpu_launch_sequence_conv.py record [path]` records the fixture: one child process per case under its own time limit,
stopping at the first that fails or whose sequence lacks an entry point its row names."""
import json
import os
import subprocess
import sys

import pytest

from test_gpu_launch_sequence_2d import launch_sequence

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "launch_sequences_conv.json")
_PLUS2D = dict(native_2d_subpixel_plus=True)
CASES = {  # name: (class, model keys, f_maps, num_groups, input shape)
    "unet2d_subpixel_plus": ("UNet2D", _PLUS2D, [8, 16, 32], 4, (2, 1, 34, 40)),  # one level n -> 2n + 1 along H only, one exact 2x
    "unet2d_subpixel_plus_hw": ("UNet2D", _PLUS2D, [8, 16, 32], 4, (2, 1, 35, 45)),  # plus along both axes, then along H only
    # the 16 -> 32 layer: split forward, fp32 data gradient; one exact-2x and one plus sub-pixel level, skip halves on u3d_conv3d_f32s
    "unet3d_f32s": ("UNet3D", dict(compute_dtype="fp32_split"), [32, 64, 128], 8, (1, 1, 9, 16, 16)),
    "unet3d_bf16": ("UNet3D", dict(compute_dtype="bf16"), [32, 64, 128], 8, (1, 1, 9, 16, 16)),  # written-out concat; 16 -> 32 stays fp32
    # post-norm order: `_bf16_vcat` and `_cat_bf16` both refuse, the decoder's first conv runs fp32 on the virtual source
    "unet2d_bf16_vcat_cgr": ("UNet2D", dict(native_2d_bf16_vcat=True, layer_order="cgr"), [32, 64], 8, (2, 1, 35, 45)),
    # the top decoder is exact 2x (`subpixel2d_bf16`), the bottom one goes 10 -> 21: its concat is written out ...
    "unet2d_bf16_subpixel": ("UNet2D", dict(native_2d_bf16_subpixel=True), [32, 64, 128], 8, (2, 1, 36, 42)),
    # ... or, with the `_src` entry points beside the sub-pixel family, read in place: no concat is written at either level
    "unet2d_bf16_subpixel_vcat": ("UNet2D", dict(native_2d_bf16_subpixel=True, native_2d_bf16_vcat=True), [32, 64, 128], 8, (2, 1, 36, 42)),
}
_SUB_BF16 = ("u3d_subpixel2d_conv_fwd_bf16", "u3d_subpixel2d_conv_dgrad_bf16", "u3d_subpixel2d_conv_wgrad_bf16")
REACHES = {  # entry points a case's sequence must contain (asserted when recording and by the test)
    "unet2d_subpixel_plus": ("u3d_subpixel2d_conv_fwd_win", "u3d_conv2d_box", "u3d_subpixel2d_conv_fwd", "u3d_conv2d_wgrad_box",
                             "u3d_nearest_childsum_add2d", "u3d_gn_bwd_apply_children2d", "u3d_chan_stats_children2d"),
    "unet2d_subpixel_plus_hw": ("u3d_subpixel2d_conv_fwd_win", "u3d_conv2d_box", "u3d_subpixel2d_conv_wgrad_win",
                                "u3d_subpixel2d_conv_dgrad_win", "u3d_conv2d_wgrad_box", "u3d_nearest_childsum_add2d"),
    "unet3d_f32s": ("u3d_conv3d_f32s", "u3d_subpixel_conv_fwd", "u3d_subpixel_conv_fwd_win", "u3d_conv3d_box",
                    "u3d_conv3d_small_cin_bwd"),
    "unet3d_bf16": ("u3d_nearest_cat_fwd", "u3d_conv3d_bf16_ex", "u3d_conv3d_wgrad_bf16_job", "u3d_conv3d_ex_reps",
                    "u3d_conv3d_wgrad_job"),
    "unet2d_bf16_vcat_cgr": ("u3d_conv2d_ex_reps", "u3d_conv2d_bf16", "u3d_conv2d_wgrad", "u3d_conv2d_wgrad_bf16"),
    "unet2d_bf16_subpixel": _SUB_BF16 + ("u3d_conv2d_bf16_res", "u3d_conv2d_wgrad_bf16_strided", "u3d_pack_subpixel2d_weights_bf16",
                                         "u3d_pack_weights2d_bf16_slice", "u3d_nearest_cat_fwd"),
    "unet2d_bf16_subpixel_vcat": _SUB_BF16 + ("u3d_conv2d_bf16_src", "u3d_conv2d_bf16_dgrad_src", "u3d_conv2d_wgrad_bf16_src"),
}
ABSENT = {"unet2d_bf16_subpixel_vcat": ("u3d_nearest_cat_fwd",)}  # entry points a case's sequence must not contain
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
    assert not {name for name, _ in got} & set(ABSENT.get(case, ())), case
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
