"""`hip_graph: true` may only be accepted next to what a test replays.  For every opt-in model key, every natively run
layer order and every natively run `upsample` value one of two things must hold: the constructor refuses the combination with an error
that names hip_graph (or the executor declines to capture it: the fallback list), or a case of the GPU case tables replays it against the
eager step (tests/test_gpu_graph.py, tests/test_gpu_graph_envelope.py; read here as data, no GPU needed).  A new key has to choose."""
import re

import pytest

import test_gpu_graph as tg
import test_gpu_graph_envelope as env
from pytorch3dunet_amd.unet3d import model as M
from pytorch3dunet_amd.unet3d import native2d
from pytorch3dunet_amd.unet3d.buildingblocks import ResNetBlock

# kwargs of every replayed case (test_gpu_graph's cases switch the flag on by hand)
REPLAYED = [kw for _, _, kw, _, _, _ in env.CASES] + [dict(kw, hip_graph=True) for _, kw, _ in tg.CASES]
# a value that switches the key on, where `True` is not one
_ON = {"compute_dtype": "bf16", "activation_dtype": "bf16", "checkpoint_levels": 1}
_BLOCK_2D = {k.name: k.block for k in native2d.KEYS}


def _smallest(key):
    """(class, kwargs) of the smallest model on which `key` means something"""
    base = dict(in_channels=1, out_channels=1, f_maps=[32, 64], num_groups=8)
    if key in native2d.NAMES:
        return (M.ResidualUNet2D if _BLOCK_2D[key] is ResNetBlock else M.UNet2D), base
    return M.UNet3D, base


@pytest.mark.parametrize("key", M._OPT_IN_KEYS)
def test_every_opt_in_key_is_refused_next_to_hip_graph_or_replayed(key):
    assert set(native2d.NAMES) <= set(M._OPT_IN_KEYS)
    if any(key in kw for kw in REPLAYED):
        return
    cls, base = _smallest(key)
    with pytest.raises(ValueError, match="hip_graph"):
        cls(**base, **{key: _ON.get(key, True)}, hip_graph=True)
    cls(**base, **{key: _ON.get(key, True)})  # (the key alone is a valid model: the refusal is of the pair)


def _params_of(module, arg):
    """every string a test of `module` is parametrised with under the argument name `arg` (alone or in a tuple of names)"""
    out = set()
    for name in dir(module):
        for mark in getattr(getattr(module, name), "pytestmark", []):
            if mark.name != "parametrize":
                continue
            argnames = [a.strip() for a in mark.args[0].split(",")] if isinstance(mark.args[0], str) else list(mark.args[0])
            if arg not in argnames:
                continue
            for value in mark.args[1]:
                value = getattr(value, "values", value)  # (pytest.param)
                v = value[argnames.index(arg)] if len(argnames) > 1 else value
                if isinstance(v, str):
                    out.add(v)
    return out


def test_every_native_layer_order_and_upsample_value_is_replayed_or_falls_back():
    import inspect

    import test_gpu_orders as orders

    native_orders = _params_of(orders, "order")
    assert {"gcl", "cge", "crg", "c", "bcr", "gcrd", "bcrD"} <= native_orders, native_orders  # (the lists were found)
    replayed = {kw.get("layer_order", "gcr") for kw in REPLAYED}
    assert not replayed & set(env.FALLBACK_ORDERS)
    missing = native_orders - replayed - set(env.FALLBACK_ORDERS)
    assert not missing, f"layer orders run natively, accepted next to hip_graph and never replayed: {sorted(missing)}"
    ups = _params_of(orders, "mode") | set(re.findall(r"upsample=\"(\w+)\"", inspect.getsource(orders))) | {"default", "nearest"}
    assert {"deconv", "trilinear", "area"} <= ups, ups
    missing = ups - {kw.get("upsample", "default") for kw in REPLAYED}
    assert not missing, f"upsample values run natively and never replayed: {sorted(missing)}"


def test_the_fallback_list_is_what_the_executor_declines():
    """every order of the fallback list is declined by `_graph_blocker`'s rule, every replayed one is not (the rule reads the order string)"""
    from pytorch3dunet_amd.engine import parse_order

    for order in env.FALLBACK_ORDERS:
        assert parse_order(order) is not None and any(ch in order for ch in "bdD"), order
    for kw in REPLAYED:
        order = kw.get("layer_order", "gcr")
        assert parse_order(order) is not None and not any(ch in order for ch in "bdD"), order


def test_case_tables_are_well_formed():
    ids = [c[0] for c in env.CASES]
    assert len(ids) == len(set(ids))
    assert len(env._UNORDERED) <= 2 and env._UNORDERED <= set(ids)
    for cid, cls, kw, loss, shapes, xgrad in env.CASES:
        assert kw["hip_graph"] is True and hasattr(M, cls)
        assert len(shapes) >= 4 and len(set(shapes)) >= 2, cid          # at least four steps over at least two shapes ...
        assert any(s in shapes[:i] for i, s in enumerate(shapes)), cid  # ... one of which returns to a shape captured earlier
        assert all(s[1] == kw.get("in_channels", 1) for s in shapes), cid
        model = getattr(M, cls)(**{**dict(in_channels=1, out_channels=1), **kw})
        assert model.hip_graph and model.native_supported, (cid, model._native_blockers)


def test_captures_collect_first_and_keep_the_cycle_collector_off():
    """`_engine_graph._quiet_gc` (around GraphStep's captures): dead reference cycles are collected on entry, the collector is off inside
    and comes back as it was — also after an exception, also when it was off before"""
    import gc
    import weakref

    from pytorch3dunet_amd._engine_graph import _quiet_gc

    class Node:
        pass

    def dead_cycle():
        a, b = Node(), Node()
        a.other, b.other = b, a
        return weakref.ref(a)

    was = gc.isenabled()
    try:
        for before in (True, False):
            (gc.enable if before else gc.disable)()
            ref = dead_cycle()
            with _quiet_gc():
                assert ref() is None and not gc.isenabled()
                inside = dead_cycle()
            assert gc.isenabled() == before and (inside() is not None or before)
            with pytest.raises(KeyError):
                with _quiet_gc():
                    raise KeyError("x")
            assert gc.isenabled() == before
    finally:
        (gc.enable if was else gc.disable)()
