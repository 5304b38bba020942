"""The opt-in model keys of the native 2-D path, resolved from ONE table (KEYS; printed in unet3d.model's docstring) into ONE record.

A 2-D model stays outside the native executor unless a key is set in the YAML's model section (`key: true`) or its environment
variable is "1" (the variable is the key's DEFAULT: an explicit `key: false` beats it).  A key means something only to the 2-D class
built from its block type; every other class ignores it entirely, a contradicting compute_dtype next to it included.  A fp32 key next
to compute_dtype bf16 WITHOUT the bf16 key of its class stays on the warning path (and next to compute_dtype fp32_split without
`native_2d_fp32_split` / `native_2d_residual_fp32_split`).  Two keys that force different precisions contradict each other.

A new key is one row of KEYS (and one kernel-family entry in _engine_conv.py); `unet3d.model` derives its keyword list from the rows."""
import dataclasses
import os
from typing import NamedTuple, Optional, Tuple

from .buildingblocks import DoubleConv, ResNetBlock


class Key(NamedTuple):
    name: str                    # model-section key
    env: str                     # the variable whose value "1" is the key's default
    block: Optional[type]        # the block type of the 2-D class it applies to (None: any 2-D class)
    implies: Optional[str]       # the key it switches on with it
    precision: Optional[str]     # the compute_dtype it forces; any other explicit compute_dtype next to it is a contradiction
    refuses: Optional[Tuple[str, str]]  # (a key it cannot stand next to, what this key is — for the error text)
    kernels: str                 # csrc file of the kernels it adds
    does: str                    # one line for the table's legend (DESIGN.md §9 has the long form)


# A key stands BEFORE the key it implies: `resolve` walks the rows once, and a contradiction names the first — the most derived — key
# that is on.  Each key is separate from the one it implies so that the implied key alone stays bit-identical.
KEYS = (
    Key("native_2d_residual_bf16_deconv", "U3D_NATIVE_2D_RESIDUAL_BF16_DECONV", ResNetBlock, "native_2d_residual_bf16", "bf16", None,
        "u3d_conv2d_bf16.hip", "also the decoders' ConvTranspose2d with both channel counts % 32 take bf16 operands, all three directions"),
    Key("native_2d_residual_bf16", "U3D_NATIVE_2D_RESIDUAL_BF16", ResNetBlock, "native_2d_residual", "bf16", None, "u3d_conv2d_bf16.hip",
        "the 3x3 layers with both channel counts % 32 take bf16 MFMA operands (fp32 residual epilogue); everything else stays fp32"),
    Key("native_2d_residual_fp32_split", "U3D_NATIVE_2D_RESIDUAL_FP32_SPLIT", ResNetBlock, "native_2d_residual", "fp32_split", None,
        "u3d_conv2d_f32s.h",
        "the 3x3 layers (conv2, conv3) of the blocks whose width is % 32 on six bf16 MFMA products of exactly split fp32 operands, all "
        "three directions, fp32-grade (fp32 residual epilogue); conv1, ConvTranspose2d and everything else stay on the fp32 kernels"),
    Key("native_2d_residual", "U3D_NATIVE_2D_RESIDUAL", ResNetBlock, "native_2d", None, None, "u3d_conv2d.hip, u3d_res.hip",
        "a fp32 ResidualUNet2D on the residual executor at D = 1; native_2d alone leaves it on the warning path"),
    Key("native_2d_bf16_vcat", "U3D_NATIVE_2D_BF16_VCAT", DoubleConv, "native_2d_bf16", "bf16", None, "u3d_conv2d_bf16.hip",
        "the decoders' first convolutions read cat(skip, interpolate(x)) in place (`_src` entry points) when both halves are % 32 channels"),
    Key("native_2d_bf16_subpixel", "U3D_NATIVE_2D_BF16_SUBPIXEL", DoubleConv, "native_2d_bf16", "bf16", None, "u3d_conv2d_bf16.hip",
        "the decoders' first convolutions at exact-2x levels with all channel counts % 32 as four 2x2 bf16 convolutions (4/9 of the MACs)"),
    Key("native_2d_bf16", "U3D_NATIVE_2D_BF16", DoubleConv, "native_2d", "bf16", None, "u3d_conv2d_bf16.hip",
        "the single-source 3x3 layers with both channel counts % 32 take bf16 MFMA operands; everything else stays fp32"),
    Key("native_2d_stem", "U3D_NATIVE_2D_STEM", DoubleConv, "native_2d", None, None, "u3d_conv2d.hip",
        "the first layer (Cin <= 4, Cout <= 32) on the small-Cin kernels, exact fp32; next to native_2d_bf16 also the % 16 layers (`_c16`)"),
    Key("native_2d_subpixel_plus", "U3D_NATIVE_2D_SUBPIXEL_PLUS", DoubleConv, "native_2d_subpixel", None, None, "u3d_subpix2d.hip, u3d_conv2d.hip",
        "also the levels that upsample n -> 2n + 1 along H and / or W: the same kernels on a shifted window + 3x3 box launches on the 2-pixel slab"),
    Key("native_2d_subpixel", "U3D_NATIVE_2D_SUBPIXEL", DoubleConv, "native_2d", None, ("native_2d_bf16", "the fp32 sub-pixel decoder path"),
        "u3d_subpix2d.hip", "the upsampled half of a decoder's first convolution at an exact-2x level as four 2x2 convolutions; no bf16 form"),
    Key("native_2d_fp32_split", "U3D_NATIVE_2D_FP32_SPLIT", DoubleConv, "native_2d", "fp32_split",
        ("native_2d_subpixel", "the fp32_split 2-D path, which has no sub-pixel kernels"), "u3d_conv2d_f32s.h",
        "the 3x3 layers with all channel counts % 32 (a decoder's virtual concat: both halves) on six bf16 MFMA products of exactly "
        "split fp32 operands, all three directions, fp32-grade; everything else stays on the fp32 kernels"),
    Key("native_2d", "U3D_NATIVE_2D", None, None, None, None, "u3d_conv2d.hip",
        "a fp32 UNet2D with nearest upsampling on the DoubleConv executor at D = 1"),
)
_BY_NAME = {k.name: k for k in KEYS}
NAMES = tuple(k.name for k in KEYS)
_DTYPE_NAMES = {"bf16": ("bf16", "bfloat16"), "fp32_split": ("fp32_split",)}  # how compute_dtype may spell a row's precision
_CLASS = {DoubleConv: "UNet2D", ResNetBlock: "ResidualUNet2D", None: "any 2-D class"}
_ROW = "  {:<30}  {:<34}  {:<14}  {:<23}  {:<10}  {}"
TABLE = "\n".join([_ROW.format("key", "variable", "class", "implies", "precision", "kernels (csrc/)")] +
                  [_ROW.format(k.name, k.env, _CLASS[k.block], k.implies or "-", k.precision or "-", k.kernels) for k in KEYS] +
                  [""] + [f"  {k.name}: {k.does}" for k in KEYS])

# the resolved keys of one model, after masking by class and implication
Native2D = dataclasses.make_dataclass("Native2D", [(n, bool, False) for n in NAMES], frozen=True)
Native2D.__module__ = __name__  # (models are pickled: torch.save(model), mp.spawn)


def _chain(key: Key) -> list:
    """`key` and every key it implies, directly or through others"""
    return [key] + (_chain(_BY_NAME[key.implies]) if key.implies else [])


def resolve(values: dict, is3d: bool, basic_module: type, compute_dtype):
    """values: {key: the constructor's keyword value, None = unset}.  Returns (Native2D, compute_dtype as the keys force it)."""
    assert set(values) <= set(NAMES), sorted(set(values) - set(NAMES))
    on, implied = [], set()
    for k in KEYS:
        v = values.get(k.name)
        if v is None:
            v = os.environ.get(k.env, "0") == "1"
        if (bool(v) or k.name in implied) and not is3d and k.block in (None, basic_module):
            on.append(k)
            implied.add(k.implies)
    forced = [k for k in on if k.precision is not None]
    for k in forced[1:]:  # (two keys that force different precisions: named as such, before either meets the other's compute_dtype)
        if k.precision != forced[0].precision:
            raise ValueError(f"u3d: {forced[0].name} runs {forced[0].precision} operands and {k.name} runs {k.precision} operands — drop "
                             "one of the two keys")
    for k in on:  # (a refusing key stands after the keys it refuses: a precision contradiction comes first)
        if k.precision is not None:
            if compute_dtype is not None and str(compute_dtype).lower() not in _DTYPE_NAMES[k.precision]:
                fp32 = next(c.name for c in _chain(k) if c.precision is None)  # the same path without the forced precision
                raise ValueError(f"u3d: {k.name} runs {k.precision} operands; compute_dtype {compute_dtype!r} contradicts it — drop one of "
                                 f"the two keys ({fp32}: true is the fp32 2-D path)")
            compute_dtype = k.precision
        if k.refuses is not None and _BY_NAME[k.refuses[0]] in on:
            other = next(o.name for o in on if k.refuses[0] in (c.name for c in _chain(o)))  # (the most derived one ...
            mine = next(o.name for o in on if k in _chain(o))  # ... on either side: a key inherits the refusal of the key it implies)
            raise ValueError(f"u3d: {mine} is {k.refuses[1]}; {other} contradicts it — drop one of the two keys")
    return Native2D(**{k.name: True for k in on}), compute_dtype
