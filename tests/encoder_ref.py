"""fp64 reference of one encoder block and an elementwise bound on what a correct fp32-accumulating route may differ from it
(test infrastructure for tests/test_encoder_blocks.py; a helper module, not a conftest).

Every convolution is im2col (F.unfold) + matmul in float64 on whatever device the input lives on: independent of MIOpen and
of the project's kernels.  The weights are the state dict's, BatchNorm folded by oracle.hmr_ref._folded (in double, then
rounded to float -- what the library's read_conv_bn + conv_pack_weights do) and, for the bf16 encoder, rounded to bf16 as
conv_pack_weights_bf16 does: the kernels multiply by exactly these weights.

The bound E travels with the reference through conv1 -> conv2 -> conv3 (+ downsample, + residual).  For z = W a + b whose
input carries a bound e_a (the route's input a' satisfies |a' - a| <= e_a):

    E_z = |W| ((1 + g) e_a + g |a|) + g (|b| + |r| + e_r)    g = gamma_K = K 2^-23,  r = a summed residual

(an fp32 dot product of K terms errs by at most ~K 2^-24 of the sum of the absolute terms; the factor 2 is slack for
the order of the MFMA's partial sums).  Wherever a route may store z, u (|z| + E_z) is added: u = 2^-8 for bf16 (the unit
roundoff of its 8-bit significand: round-to-nearest-even errs by at most u |z|, with no slack -- the stem, where nothing
else enters, reaches r = 0.986 on the MI355X), 2^-23 for fp32 (twice its unit roundoff).  ReLU and max-pool are 1-Lipschitz and pass E through.  The t1 / t2
intermediates and the downsample branch always get the storage term, so the bound does not depend on which route -- a
whole-block kernel, a dual-source GEMM, a fused conv2 + conv3 -- the plan took.

fp32 Winograd layers.  A componentwise bound of F(m x m, 3x3) is not a multiple of the direct one: the output transform
mixes every input of the (m+2)^2 tile into every output, so no constant C_m times gamma_K |W| |a| bounds it (the
rigorous form is a different abs-value operator, with terms |A^T| (|G| |g| |G^T| . |B^T| |d| |B|) |A| whose growth for
F(4x4) on five points is what Winograd's accuracy literature measures).  For those layers the bound takes the norm-wise
criterion of tests/test_hip_parity.py::test_conv_winograd_matches_torch_and_direct instead: 2e-5 of the frame's largest
|W| |a| + |b| (>= its largest |z|) is added to E_z2 of every element of that frame, and propagates through conv3.
"""
import torch
import torch.nn.functional as F

from oracle import hmr_ref

U_BF16 = 2.0 ** -8
U_F32 = 2.0 ** -23
WINO_TOL = 2e-5          # test_conv_winograd_matches_torch_and_direct's criterion, relative to the layer's scale
TILE = 32                # RMS tiles: 32 pixels (row-major within a frame) x 32 channels
# bound on every tile's RMS of r = (route - reference) / E relative to its block's RMS of r (Stats).  Measured on the
# MI355X over every block of the nine configurations of test_encoder_blocks.py: 2.14 at most (fp32 Winograd, block 12;
# bf16 2.03); 3 leaves 1.4x.
RHO = 3.0


def gamma(K):
    return K * 2.0 ** -23


class Conv:
    """One folded convolution in float64: w [Cout, Cin, k, k], b [Cout]."""

    def __init__(self, w, b, stride=1, pad=0):
        self.w, self.b, self.stride, self.pad = w, b, stride, pad
        self.k = w.shape[-1]
        self.K = w.shape[1] * self.k * self.k
        self.wabs = w.abs()

    def to(self, device):
        return Conv(self.w.to(device), self.b.to(device), self.stride, self.pad)


def folded_conv(conv, bn, bf16, device="cpu"):
    with torch.no_grad():
        w, b = hmr_ref._folded(conv, bn)
    if bf16:
        w = hmr_ref._bf16(w)
    return Conv(w.double().to(device), b.double().to(device), conv.stride[0], conv.padding[0])


def _mm(a, w, stride, pad):
    """conv2d(a, w) without bias as im2col + matmul, in a's dtype (NCHW)."""
    N, _, H, W = a.shape
    k = w.shape[-1]
    Ho, Wo = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
    if k == 1:
        a = a[:, :, ::stride, ::stride] if stride > 1 else a
        return torch.einsum("nchw,oc->nohw", a, w[:, :, 0, 0])
    cols = F.unfold(a, k, padding=pad, stride=stride)                     # [N, Cin k k, L]
    return (w.reshape(w.shape[0], -1) @ cols).reshape(N, w.shape[0], Ho, Wo)


def conv_bound(c, a, e_a, extra_k=0):
    """-> (z = W a + b, E_z without the residual and storage terms).  extra_k: K of a second source summed in the same
    K loop (a first block's downsample rides in conv3's), which lengthens the sum gamma is taken over."""
    g = gamma(c.K + extra_k + 1)
    z = _mm(a, c.w, c.stride, c.pad) + c.b.view(1, -1, 1, 1)
    src = g * a.abs() if e_a is None else (1 + g) * e_a + g * a.abs()
    E = _mm(src, c.wabs, c.stride, c.pad) + g * c.b.abs().view(1, -1, 1, 1)
    return z, E


def stored(y, E, u):
    return E + u * (y.abs() + E)


class Block:
    """conv1 / conv2 / conv3 (+ downsample) of one Bottleneck, folded, in float64."""

    def __init__(self, blk, bf16, device="cpu"):
        self.c1 = folded_conv(blk.conv1, blk.bn1, bf16, device)
        self.c2 = folded_conv(blk.conv2, blk.bn2, bf16, device)
        self.c3 = folded_conv(blk.conv3, blk.bn3, bf16, device)
        self.cd = folded_conv(blk.downsample[0], blk.downsample[1], bf16, device) if blk.downsample is not None else None


def block_ref(p, a, u, wino=False):
    """Reference output and bound of one Bottleneck from its exact input a (NCHW float64)."""
    z1, E1 = conv_bound(p.c1, a, None)
    t1 = z1.clamp_min(0)
    E1 = stored(t1, E1, u)
    z2, E2 = conv_bound(p.c2, t1, E1)
    if wino:
        scale = (_mm(t1.abs() + E1, p.c2.wabs, 1, 1) + p.c2.b.abs().view(1, -1, 1, 1)).amax(dim=(1, 2, 3), keepdim=True)
        E2 = E2 + WINO_TOL * scale.clamp_min(1.0)
    t2 = z2.clamp_min(0)
    E2 = stored(t2, E2, u)
    if p.cd is not None:
        kd = p.cd.K
        d, Ed = conv_bound(p.cd, a, None, extra_k=p.c3.K)
        Ed = stored(d, Ed, u)
        z3, E3 = conv_bound(p.c3, t2, E2, extra_k=kd)
        g = gamma(p.c3.K + kd + 1)
        idt, Eidt = d, Ed
    else:
        z3, E3 = conv_bound(p.c3, t2, E2)
        g = gamma(p.c3.K + 1)
        idt, Eidt = a, torch.zeros_like(a)
    z3 = z3 + idt
    E3 = E3 + Eidt + g * (idt.abs() + Eidt)
    y = z3.clamp_min(0)
    return y, stored(y, E3, u)


def stem_ref(c, x, u):
    """conv1 + bn1 + ReLU, stored, then the 3x3 / stride-2 max-pool (which takes E through as a max over the window)."""
    z, E = conv_bound(c, x, None)
    y = z.clamp_min(0)
    E = stored(y, E, u)
    return F.max_pool2d(y, 3, 2, 1), F.max_pool2d(E, 3, 2, 1)


def pool_ref(y):
    """Global average pool of the last block's output (NCHW float64) -> (features, bound): a sum of 49 fp32 terms, then
    one rounding of the mean."""
    f = y.mean(dim=(2, 3))
    return f, gamma(y.shape[2] * y.shape[3] + 1) * y.abs().mean(dim=(2, 3)) + U_F32 * f.abs()


class Reference:
    """The folded network of a SPIN state dict: stem + 16 Bottlenecks, float64 on `device`."""

    def __init__(self, state_dict, precision, device):
        m = hmr_ref.build(state_dict)
        bf = precision == "bf16"
        self.u = U_BF16 if bf else U_F32
        self.bf16 = bf
        self.stem = folded_conv(m.conv1, m.bn1, bf, device)
        self.blocks = [Block(b, bf, device) for stage in (m.layer1, m.layer2, m.layer3, m.layer4) for b in stage]

    def block(self, k, a, wino_form=0):
        """Block k (1..16) from its input a (NCHW float64): (y, E).  wino_form: the fp32 handle's Winograd form, which
        covers the stride-1 3x3 convolutions with >= 128 channels (layer2..layer4 past their first block)."""
        p = self.blocks[k - 1]
        wino = bool(wino_form) and p.c2.stride == 1 and p.c2.w.shape[1] >= 128
        return block_ref(p, a, self.u, wino)

    def block0(self, x):
        """Stem + max-pool from the NCHW input (rounded to bf16 for the bf16 encoder, as its layout change does)."""
        x = x.double()
        if self.bf16:
            x = hmr_ref._bf16(x.float()).double()
        return stem_ref(self.stem, x, self.u)


def ratios(gpu, ref, E):
    """r = (gpu - ref) / E elementwise (NCHW float64; 0 where both the difference and the bound are 0)."""
    d = (gpu - ref).abs()
    r = d / E.clamp_min(1e-300)
    return torch.where(d == 0, torch.zeros_like(r), r)


def tile_rms(r):
    """RMS of r over every 32-pixel x 32-channel output tile of each frame (pixels row-major; a frame's last tile may be
    ragged) -> [N, pixel tiles, channel tiles]."""
    N, C, H, W = r.shape
    P = H * W
    q = r.permute(0, 2, 3, 1).reshape(N, P, C) ** 2
    pad = (-P) % TILE
    n = torch.full((P + pad,), 1.0, dtype=r.dtype, device=r.device)
    if pad:
        q = F.pad(q, (0, 0, 0, pad))
        n[P:] = 0
    s = q.reshape(N, (P + pad) // TILE, TILE, C // TILE, TILE).sum(dim=(2, 4))
    cnt = n.reshape(-1, TILE).sum(1).view(1, -1, 1) * TILE
    return (s / cnt).sqrt()


class Stats:
    """max |r| and the tile RMS of r, accumulated over a block's frame chunks.  The tile criterion is relative: no tile's
    RMS of r exceeds RHO times the block's RMS of r over all its elements.  How much of E a correct route uses differs by
    block (the stem's r is its one rounding, ~0.3; a bf16 block's ~0.01 behind the propagated t1 / t2 terms; fp32 ~1e-5), so
    an absolute level would be either blind or wrong somewhere; a defect confined to one tile, one chunk or one channel
    stands out against its own block."""

    def __init__(self):
        self.max_r, self.max_tile, self.sq, self.n = 0.0, 0.0, 0.0, 0

    def add(self, gpu, ref, E):
        r = ratios(gpu, ref, E)
        self.max_r = max(self.max_r, float(r.max()))
        self.max_tile = max(self.max_tile, float(tile_rms(r).max()))
        self.sq += float((r * r).sum())
        self.n += r.numel()
        return self

    @property
    def tile_ratio(self):
        rms = (self.sq / max(self.n, 1)) ** 0.5
        return self.max_tile / rms if rms > 0 else 0.0


def check_stats(gpu, ref, E):
    """-> (max |r|, largest tile RMS of r / the block's RMS of r) of one block (NCHW float64 tensors)."""
    s = Stats().add(gpu, ref, E)
    return s.max_r, s.tile_ratio
