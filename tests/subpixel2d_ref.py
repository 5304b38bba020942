"""TEST HELPER (not a test): the sub-pixel identities that csrc/u3d_subpix2d.hip builds on, restated for 2-D in plain torch tensor
algebra after oracle/subpixel_oracle.py.  Nothing under pytorch-3dunet_amd/ imports this module.

The reference computes, for the upsampled half of a decoder's first convolution of a UNet2D (buildingblocks.py:491 torch.cat, :614
F.interpolate(mode='nearest'), :55-58 nn.Conv2d(k=3, padding=1)):

    y = conv2d(nearest2x(low), w)                                   full-res, 9 taps per output pixel

Per axis, output pixel 2j + p reads low-res pixels j + p - 1 + e, e in {0, 1}, with the taps that hit the same low-res pixel summed:
p=0: e=0 <- {t0}, e=1 <- {t1, t2};   p=1: e=0 <- {t0, t1}, e=1 <- {t2}.
"""
import itertools

import torch
import torch.nn.functional as F

# taps of parity p that read low-res offset (p - 1 + e)
TAPS = {(0, 0): (0,), (0, 1): (1, 2), (1, 0): (0, 1), (1, 1): (2,)}


def presum_weights(w):
    """w (Cout, C1, 3, 3) -> dict[(py,px)] = (Cout, C1, 2, 2): the 2x2 kernel of every output parity class"""
    out = {}
    for p in itertools.product((0, 1), repeat=2):
        k = torch.zeros(w.shape[0], w.shape[1], 2, 2, dtype=w.dtype)
        for e in itertools.product((0, 1), repeat=2):
            for ty in TAPS[(p[0], e[0])]:
                for tx in TAPS[(p[1], e[1])]:
                    k[:, :, e[0], e[1]] += w[:, :, ty, tx]
        out[p] = k
    return out


def _shifted(low, p):
    """zero-padded low-res tensor such that a VALID 2x2 correlation yields, at j, the sum over e of low[j + p - 1 + e]"""
    return F.pad(low, [1 - p[1], p[1], 1 - p[0], p[0]])  # F.pad order: last dimension first


def forward(low, w):
    """4 parity-class 2x2 convolutions over the low-res grid, interleaved into the full-res output"""
    N, C1, H1, W1 = low.shape
    y = torch.zeros(N, w.shape[0], 2 * H1, 2 * W1, dtype=low.dtype)
    for p, k in presum_weights(w).items():
        y[:, :, p[0]::2, p[1]::2] = F.conv2d(_shifted(low, p), k)
    return y


def dgrad_low(dz, w):
    """gradient with respect to `low` (children sum of the nearest upsampling included): adjoint of forward()"""
    N, K, H, W = dz.shape
    H1, W1 = H // 2, W // 2
    dlow = torch.zeros(N, w.shape[1], H1, W1, dtype=dz.dtype)
    for p, k in presum_weights(w).items():
        g = F.conv_transpose2d(dz[:, :, p[0]::2, p[1]::2], k)  # gradient of the padded tensor
        dlow += g[:, :, 1 - p[0]:1 - p[0] + H1, 1 - p[1]:1 - p[1] + W1]
    return dlow


def wgrad(low, dz):
    """dw (Cout, C1, 3, 3) from the 16 (class, tap half) matrices, folded 4 per tap"""
    N, C1, H1, W1 = low.shape
    dw = torch.zeros(dz.shape[1], C1, 3, 3, dtype=low.dtype)
    for p in itertools.product((0, 1), repeat=2):
        dzp = dz[:, :, p[0]::2, p[1]::2]
        lp = _shifted(low, p)
        for e in itertools.product((0, 1), repeat=2):
            a = lp[:, :, e[0]:e[0] + H1, e[1]:e[1] + W1]
            m = torch.einsum("nkyx,ncyx->kc", dzp, a)  # dWc[p][e]
            for ty in TAPS[(p[0], e[0])]:
                for tx in TAPS[(p[1], e[1])]:
                    dw[:, :, ty, tx] += m
    return dw


# per axis: the taps that dz[2j - 1 + e], e = 0..3, carries in the gradient of low[j] (the data-gradient image of the library)
DGRAD_TAPS = ((2,), (1, 2), (0, 1), (0,))


def dgrad_low_gather(dz, w):
    """the same gradient as the 4 x 4-tap, stride-2 gather of dz that u3d_subpixel2d_conv_dgrad_reps evaluates"""
    N, K, H, W = dz.shape
    H1, W1 = H // 2, W // 2
    dzp = F.pad(dz, [1, 1, 1, 1])
    dlow = torch.zeros(N, w.shape[1], H1, W1, dtype=dz.dtype)
    for ey, ex in itertools.product(range(4), repeat=2):
        k = sum(w[:, :, ty, tx] for ty in DGRAD_TAPS[ey] for tx in DGRAD_TAPS[ex])  # (Cout, C1)
        dlow += torch.einsum("nkyx,kc->ncyx", dzp[:, :, ey:ey + 2 * H1:2, ex:ex + 2 * W1:2], k)
    return dlow
