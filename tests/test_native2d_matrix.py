"""The interaction matrix of the eight `native_2d*` model keys, exhaustively, against what the commit before the keys were resolved from
one table computed (tests/golden/native2d_key_matrix.json).

  keys     5 classes x compute_dtype {absent, fp32, bf16, fp32_split} x every subset of the eight keys set to True: 5120 constructions at
           f_maps [8, 16], num_groups 4
  env      each environment variable alone set to "1" x 5 classes x its key {absent, False} x compute_dtype {absent, fp32}: 160

A case is either the constructor's error (type name and text) or the model's eleven resolved attributes.  A case that is a
native-supported 2-D model is built again at f_maps [16, 32, 64], num_groups 8 (where the % 16 / % 32 routing rules have both outcomes)
and its executor — built on the CPU, which needs the library and no GPU — adds its flags, the shapes of the weights in its 2-D image
lists, its virtual-concat weights and the number of sub-pixel layers at an exact-2x and at an odd input size.

The fixture holds the distinct outcomes once and one index per case.  `python tests/test_native2d_matrix.py` records it."""
import itertools
import json
import os

import pytest

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "native2d_key_matrix.json")
CLASSES = ("UNet3D", "ResidualUNet3D", "ResidualUNetSE3D", "UNet2D", "ResidualUNet2D")
KEYS = ("native_2d", "native_2d_residual", "native_2d_bf16", "native_2d_residual_bf16", "native_2d_residual_bf16_deconv",
        "native_2d_stem", "native_2d_bf16_vcat", "native_2d_subpixel")
ENV = {k: "U3D_" + k.upper() for k in KEYS}
DTYPES = (None, "fp32", "bf16", "fp32_split")
ATTRS = ("native_2d", "native_2d_stem", "native_2d_subpixel", "native_2d_bf16", "native_2d_bf16_vcat", "native_2d_residual_bf16",
         "native_2d_residual_bf16_deconv", "compute_bf16", "compute_split", "native_supported", "_native_blockers")
ENGINE_FLAGS = ("is2d", "stem", "subpixel2d", "subpixel", "children", "vcat", "bf16_deconv", "bf16", "split")
SMALL = dict(in_channels=1, out_channels=1, f_maps=[8, 16], num_groups=4)
WIDE = dict(in_channels=1, out_channels=1, f_maps=[16, 32, 64], num_groups=8)
# every variable a constructor or an executor reads its defaults from: the matrix is recorded and replayed with none of them set
_CLEAN = tuple(ENV.values()) + ("U3D_BF16", "U3D_F32_SPLIT", "U3D_GRAPH", "U3D_CHECKPOINT", "U3D_CHECKPOINT_LEVELS", "U3D_ACT_BF16",
                                "U3D_SUBPIXEL", "U3D_SUBPIXEL_PLUS", "U3D_BF16_CAT", "U3D_STAT_REPS")


def key_cases():
    """the `keys` axis of every class: (compute_dtype, the keys set to True)"""
    for dtype in DTYPES:
        for bits in itertools.product((False, True), repeat=len(KEYS)):
            yield dtype, tuple(k for k, on in zip(KEYS, bits) if on)


def env_cases():
    """the `env` axis: (variable's key, class, keyword arguments)"""
    for key in KEYS:
        for name in CLASSES:
            for explicit in ({}, {key: False}):
                for dtype in (None, "fp32"):
                    yield key, name, dict(explicit, **({} if dtype is None else {"compute_dtype": dtype}))


def _engine_record(eng):
    shapes = lambda ws: [list(w.shape) for w in ws]  # noqa: E731
    im = eng.images
    virtual = sorted(list(m.weight.shape) for m in eng.model.modules() if id(getattr(m, "weight", None)) in eng._virtual_w)
    flags = {f: getattr(eng, f) for f in ENGINE_FLAGS}
    assert all(type(v) in (bool, float) for v in flags.values()), flags
    return dict(flags=flags, each=shapes(im._each), each_bf16=shapes(im._each_bf16), each_bf16_c16=shapes(im._each_bf16_c16),
                virtual_w=[len(eng._virtual_w), virtual],
                subpixel_layers=[len(eng._subpixel_layers((1, 36, 40))), len(eng._subpixel_layers((1, 35, 45)))])


def outcome(name, kwargs):
    from pytorch3dunet_amd.unet3d import model as M

    cls = getattr(M, name)
    try:
        m = cls(**SMALL, **kwargs)
    except Exception as e:  # noqa: BLE001 - the error IS the outcome
        return {"error": type(e).__name__, "msg": str(e)}
    out = {a: getattr(m, a) for a in ATTRS}
    assert all(type(out[a]) is bool for a in ATTRS[:-1]), out  # (plain bools: callers test `is False`)
    out["_native_blockers"] = list(out["_native_blockers"])
    if m.native_supported and not m._is3d:
        out["engine"] = _engine_record(cls(**WIDE, **kwargs)._get_engine())
    return out


def _kw(dtype, on):
    return dict({k: True for k in on}, **({} if dtype is None else {"compute_dtype": dtype}))


def record():
    for v in _CLEAN:
        os.environ.pop(v, None)
    outcomes, index = [], {}

    def idx(o):
        s = json.dumps(o, sort_keys=True)
        if s not in index:
            index[s] = len(outcomes)
            outcomes.append(o)
        return index[s]

    keys = {name: [idx(outcome(name, _kw(dtype, on))) for dtype, on in key_cases()] for name in CLASSES}
    env = []
    for key, name, kwargs in env_cases():
        os.environ[ENV[key]] = "1"
        try:
            env.append(idx(outcome(name, kwargs)))
        finally:
            del os.environ[ENV[key]]
    with open(FIXTURE, "w") as fh:
        json.dump({"outcomes": outcomes, "keys": keys, "env": env}, fh, separators=(",", ":"), sort_keys=True)
        fh.write("\n")
    n = sum(len(v) for v in keys.values())
    errors = sum("error" in outcomes[i] for v in keys.values() for i in v)
    print(f"{n} + {len(env)} cases, {errors} of the first axis raise, {len(outcomes)} distinct outcomes -> {FIXTURE}")


@pytest.fixture(scope="module")
def fixture():
    with open(FIXTURE) as fh:
        return json.load(fh)


@pytest.fixture
def clean_env(monkeypatch):
    for v in _CLEAN:
        monkeypatch.delenv(v, raising=False)
    return monkeypatch


def _same(got, want):
    return json.dumps(got, sort_keys=True) == json.dumps(want, sort_keys=True)


@pytest.mark.parametrize("name", CLASSES)
def test_every_subset_of_the_keys(name, fixture, clean_env):
    want = fixture["keys"][name]
    cases = list(key_cases())
    assert len(cases) == len(want) == len(DTYPES) * 2 ** len(KEYS)
    bad = []
    for (dtype, on), i in zip(cases, want):
        got = outcome(name, _kw(dtype, on))
        if not _same(got, fixture["outcomes"][i]):
            bad.append((dtype, on, got, fixture["outcomes"][i]))
    assert not bad, f"{len(bad)} of {len(cases)} constructions differ; the first: {bad[0]}"


def test_every_environment_default(fixture, clean_env):
    cases = list(env_cases())
    assert len(cases) == len(fixture["env"]) == 160
    bad = []
    for (key, name, kwargs), i in zip(cases, fixture["env"]):
        clean_env.setenv(ENV[key], "1")
        got = outcome(name, kwargs)
        clean_env.delenv(ENV[key])
        if not _same(got, fixture["outcomes"][i]):
            bad.append((ENV[key], name, kwargs, got, fixture["outcomes"][i]))
    assert not bad, f"{len(bad)} of {len(cases)} constructions differ; the first: {bad[0]}"


if __name__ == "__main__":
    import sys

    _root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.join(_root, "pytorch-3dunet_amd"))
    record()
