"""What the reference computed in the tests that compare against it, read from tests/golden/r*_*.npz (written by
tests/golden/make_reference_records.py from the live reference).  Case tables live here so that the generator and the
tests agree on seeds, configurations and shapes."""
import hashlib
import json
import os

import numpy as np
import torch

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
# gradient tensors of more than FULL_GRAD elements are recorded as every GRAD_STRIDE-th element plus their max|g|
FULL_GRAD = 512
GRAD_STRIDE = 16

# tests/test_oracle.py, one table per test
LIVE_CASES = [
    (dict(name="UNet3D", in_channels=1, out_channels=1, f_maps=16, num_groups=8), (1, 1, 17, 33, 33)),
    (dict(name="UNet3D", in_channels=3, out_channels=2, f_maps=[8, 16, 32], num_groups=4, final_sigmoid=False), (2, 3, 8, 16, 12)),
]
ORDERS = ["gcl", "gce", "cgr", "cgl", "cge", "cg", "gc", "crg", "clg", "ceg"]
RESIDUAL_ORDERS = ["cge", "cgr", "gcl", "gce", "cgl", "gc", "cg", "crg", "ceg"]
BN_ORDERS = ["bcr", "cbr", "crb", "cbl", "cr", "cl", "ce", "c"]
DECONV_NAMES = ["ResidualUNet3D", "ResidualUNetSE3D"]
INTERP_MODES = ["trilinear", "area"]
# tests/test_boundary.py::test_state_dict_keys_shapes_match_reference
STATE_DICT_CFGS = [
    dict(name="UNet3D", in_channels=1, out_channels=1, f_maps=16),
    dict(name="UNet3D", in_channels=3, out_channels=2, f_maps=[16, 32, 64], num_groups=4, final_sigmoid=False),
    dict(name="ResidualUNet3D", in_channels=1, out_channels=1, f_maps=16),
    dict(name="ResidualUNetSE3D", in_channels=1, out_channels=1, f_maps=16, num_levels=3),
    dict(name="UNet2D", in_channels=1, out_channels=1, f_maps=16),
    dict(name="ResidualUNet2D", in_channels=1, out_channels=1, f_maps=16, num_levels=3),
]


def digest(t):
    return hashlib.sha256(t.detach().contiguous().numpy().tobytes()).hexdigest()


def state_dict_id(cfg):
    return cfg["name"] + str(cfg["in_channels"])


def model_cases():
    """{file name: {case id: (seed, cfg, input shape, loss, train)}}"""
    pair = dict(in_channels=2, out_channels=2, num_groups=4, final_sigmoid=False)
    return {
        "r1_reference_unet3d": {
            **{f"live/{i}": (7, cfg, shape, "bce_dice", False) for i, (cfg, shape) in enumerate(LIVE_CASES)},
            **{f"ordered/{o}": (11, dict(name="UNet3D", f_maps=[8, 16], layer_order=o, **pair), (1, 2, 8, 12, 10), "probs_sum", False)
               for o in ORDERS},
            **{f"interp/{m}": (17, dict(name="UNet3D", f_maps=[8, 16, 32], upsample=m, **pair), (1, 2, 9, 13, 12), "probs_sum", False)
               for m in INTERP_MODES},
        },
        "r4_reference_batchnorm": {
            f"bn/{n}/{o}": (19, dict(name=n, f_maps=[8, 16], layer_order=o, **pair), (2, 2, 8, 12, 10), "probs_sum", True)
            for n in ("UNet3D", "ResidualUNet3D") for o in BN_ORDERS
        },
        "r2_reference_resunet3d": {
            **{f"residual/ResidualUNet3D/{o}": (13, dict(name="ResidualUNet3D", f_maps=[8, 16, 32], layer_order=o, **pair),
                                                (1, 2, 8, 12, 12), "probs_sum", False) for o in RESIDUAL_ORDERS},
            "deconv/ResidualUNet3D": (23, dict(name="ResidualUNet3D", f_maps=[8, 16, 32], upsample="deconv", **pair), (1, 2, 9, 12, 10),
                                      "probs_sum", False),
        },
        "r3_reference_resunetse3d": {
            **{f"residual/ResidualUNetSE3D/{o}": (13, dict(name="ResidualUNetSE3D", f_maps=[8, 16, 32], layer_order=o, **pair),
                                                  (1, 2, 8, 12, 12), "probs_sum", False) for o in RESIDUAL_ORDERS},
            "deconv/ResidualUNetSE3D": (23, dict(name="ResidualUNetSE3D", f_maps=[8, 16, 32], upsample="deconv", **pair), (1, 2, 9, 12, 10),
                                        "probs_sum", False),
        },
    }




def predictor_inputs():
    """the models and volumes of the predictor comparison, drawn in a fixed order from fixed seeds: ({case: (model, cout, raw,
    patch, stride, halo, mean, std, predictor kwargs)}, (model, raw, patch, stride, halo, mean, std, ground truth) of the dice
    case).  Models are this project's UNet3D (seeded init, module tree on the CPU)."""
    from pytorch3dunet_amd.unet3d.model import UNet3D

    torch.manual_seed(0)
    rng = np.random.RandomState(0)
    cases = {}
    for case, (cin, cout, shape, patch, stride, halo, kw) in {
        "probs": (1, 2, (20, 33, 29), (8, 16, 16), (6, 12, 12), (2, 4, 4), {}),
        "channel": (1, 3, (16, 24, 24), (8, 16, 16), (8, 8, 8), (0, 0, 0), {"prediction_channel": 1}),
        "segm_multi": (2, 3, (16, 24, 24), (8, 16, 16), (8, 16, 16), (2, 2, 2), {"save_segmentation": True}),
        "segm_single": (1, 1, (16, 24, 24), (8, 16, 16), (8, 16, 16), (2, 2, 2), {"save_segmentation": True}),
    }.items():
        model = UNet3D(cin, cout, f_maps=[4, 8], num_groups=2, final_sigmoid=(cout == 1)).eval()
        raw = rng.randn(*((cin,) + shape if cin > 1 else shape)).astype(np.float32) * 3 + 1
        cases[case] = (model, cout, raw, patch, stride, halo, float(raw.mean()), float(raw.std()), kw)
    model = UNet3D(1, 2, f_maps=[4, 8], num_groups=2, final_sigmoid=True).eval()
    raw = rng.randn(16, 24, 24).astype(np.float32)
    gt = (rng.rand(2, 16, 24, 24) > 0.5).astype(np.uint16)
    return cases, (model, raw, (8, 16, 16), (8, 8, 8), (0, 0, 0), 0.0, 1.0, gt)


_cache = {}


def record(fname):
    if fname not in _cache:
        _cache[fname] = np.load(os.path.join(GOLDEN_DIR, fname + ".npz"), allow_pickle=False)
    return _cache[fname]


class ModelRun:
    """one recorded reference run: `sd` is the state_dict BEFORE the forward (our seeded init, equal to the reference's), `x` and
    `target` are redrawn from the same seed (checked against the reference's digests), `probs` / `logits` / `buffers` (after the
    training forward) are what the reference computed; `grad_rel_err` compares a gradient with the reference's"""

    def __init__(self, case_id):
        fname = next(f for f, cases in model_cases().items() if case_id in cases)
        z, pre = record(fname), case_id + "/"
        self.seed, self.cfg, self.shape, self.loss, self.train = model_cases()[fname][case_id]
        self.keys = [str(k) for k in z[pre + "keys"]]
        t = lambda k: torch.from_numpy(np.array(z[pre + k]))  # noqa: E731
        self.probs, self.logits = t("probs"), t("logits")
        # recorded gradients in parameter order: name -> (stride, values at flatten()[::stride], max|g| of the whole tensor)
        self.grads = {}
        for k in z.files:
            if k.startswith(pre + "grad/"):
                g = t(k[len(pre):])
                self.grads[k[len(pre) + 5:]] = (1, g.flatten(), g.abs().max().item())
            elif k.startswith(pre + "grad_s/"):
                name = k[len(pre) + 7:]
                self.grads[name] = (GRAD_STRIDE, t(k[len(pre):]), float(z[pre + "grad_absmax/" + name]))
        self.buffers = {k[len(pre) + 4:]: t(k[len(pre):]) for k in z.files if k.startswith(pre + "buf/")}
        from pytorch3dunet_amd.unet3d.model import get_model

        torch.manual_seed(self.seed)
        self.sd = {k: v.detach().clone() for k, v in get_model(dict(self.cfg)).state_dict().items()}
        assert list(self.sd) == self.keys, f"{case_id}: state_dict keys differ from the reference's"
        # the reference drew x (and the target) right after its seeded init, which consumes the stream as ours does
        self.x = torch.randn(self.shape)
        if self.loss == "bce_dice":  # drawn after the forward, from the logits' shape
            self.target = (torch.rand(self.logits.shape) > 0.5).float()
        else:
            self.target = (torch.rand(self.shape[:1] + (self.cfg["out_channels"],) + self.shape[2:]) > 0.5).float()
        assert digest(self.x) == str(z[pre + "x_sha256"]), f"{case_id}: input differs from the reference's"
        assert digest(self.target) == str(z[pre + "target_sha256"]), f"{case_id}: target differs from the reference's"

    def grad_rel_err(self, name, grad):
        """max|ours - reference| / max|reference| over the recorded elements (all of them, or every GRAD_STRIDE-th of a large
        tensor: the denominator is the whole tensor's max|g| either way) — unet3d_oracle.rel_err on what the record holds"""
        stride, ref, absmax = self.grads[name]
        assert (grad.numel() + stride - 1) // stride == ref.numel(), name
        err = (grad.detach().flatten()[::stride].to(ref.dtype) - ref).abs().max().item()
        return err / (absmax if absmax > 0 else 1.0)


def misc(key):
    v = record("r0_reference_misc")[key]
    return json.loads(str(v)) if v.dtype.kind == "U" else np.array(v)
