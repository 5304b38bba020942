"""What the reference computes for seeded ResidualUNet2D runs, read from tests/golden/r7_reference_resunet2d.npz (written by
tests/golden/make_reference_resunet2d.py from the live reference).  The case table lives here so that the generator and the tests agree
on seeds, configurations and shapes.  2 x 1 x 67 x 45 inputs: the pools floor (67 -> 33 -> 16, 45 -> 22 -> 11) and the transposed
convolutions' 2n - 1 outputs are resized to the skip by both ratios (16 -> 31 -> 33, 33 -> 65 -> 67, 11 -> 21 -> 22, 22 -> 43 -> 45).
The record layout is the one of tests/reference_records_2d.py."""
import numpy as np
import torch

from reference_records import GRAD_STRIDE, digest, record  # noqa: F401

FNAME = "r7_reference_resunet2d"
SHAPE = (2, 1, 67, 45)
_BASE = dict(name="ResidualUNet2D", in_channels=1, out_channels=1, f_maps=[8, 16, 32], num_groups=4)
CASES = {
    "gcr": (51, dict(_BASE, layer_order="gcr")),
    "cge": (53, dict(_BASE, layer_order="cge")),  # ELU after `out += residual`
    "bcr": (57, dict(_BASE, layer_order="bcr")),  # BatchNorm running statistics recorded too
    "deconv": (59, dict(_BASE, layer_order="gcr", upsample="deconv")),  # explicit deconv: concat joining + the block's 1x1 conv
    "softmax": (61, dict(_BASE, out_channels=2, final_sigmoid=False, layer_order="gcr")),
}


class RunRes2D:
    """one recorded reference run (train mode, BCEDice on the logits): `sd` = the seeded init (ours equals the reference's), `x` and
    `target` redrawn from the seed and checked against the reference's digests; `probs`, `logits`, `loss`, `grads` (name -> (stride,
    recorded values, max|g|)) and `buffers` (BatchNorm running statistics after the forward) as the reference computed them"""

    def __init__(self, case_id):
        z, pre = record(FNAME), case_id + "/"
        self.seed, self.cfg = CASES[case_id]
        self.shape = SHAPE
        t = lambda k: torch.from_numpy(np.array(z[pre + k]))  # noqa: E731
        self.probs, self.logits, self.loss = t("probs"), t("logits"), float(z[pre + "loss"])
        self.keys = [str(k) for k in z[pre + "keys"]]
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
        self.x = torch.randn(self.shape)
        self.target = (torch.rand(self.logits.shape) > 0.5).float()
        assert digest(self.x) == str(z[pre + "x_sha256"]), f"{case_id}: input differs from the reference's"
        assert digest(self.target) == str(z[pre + "target_sha256"]), f"{case_id}: target differs from the reference's"

    def grad_rel_err(self, name, grad):
        """max|ours - reference| / max|reference| over the recorded elements"""
        stride, ref, absmax = self.grads[name]
        assert (grad.numel() + stride - 1) // stride == ref.numel(), name
        err = (grad.detach().flatten()[::stride].to(ref.dtype) - ref).abs().max().item()
        return err / (absmax if absmax > 0 else 1.0)
