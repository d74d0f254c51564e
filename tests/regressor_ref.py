"""fp64 reference of one regressor launch (fc_rows16_f32, csrc/fc_regressor.hip) from that launch's own input, an
elementwise bound on what a correct fp32 route may differ from it, and the kernel's arithmetic emulated in fp32 as the
yardstick of its error level (test infrastructure for tests/test_regressor_steps.py and tests/test_regressor_checker.py; a
helper module, not a conftest).

The ten launches of a batch (pr_hmr_regress_until's steps 1..10; step 0 is the state's initial value):

    1        fc1x   h_static = xf W1x^T + b1                 K 2048, N 1024
    2 + 3 i  fc1s   h1 = state W1s^T + h_static              K 192 (157 real), N 1024
    3 + 3 i  fc2    h2 = h1 W2^T + b2                        K 1024, N 1024
    4 + 3 i  dec    state = h2 Wdec^T + bdec + state         K 1024, N 192 (157 real), in place

The weights are the state dict's, arranged as host_plan.cc::make_fc does: fc1 split at column 2048, decpose | decshape |
deccam stacked, rows and columns padded with zeros to 192.

Why one launch at a time.  A worst-case bound carried through the launches, the way encoder_ref carries E through a block, is
blind here: the products |W| |a| have no cancellation and nine layers of them put E on the final state at hundreds for values
of a few units (tests/test_regressor_checker.py asserts it).  From its own input one GEMM's bound is useful:

    E = (K + 2) 2^-23 (|W| |a| + |b| + |res|) + 2^-23 |z|

(an fp32 dot product of K terms errs by at most ~K 2^-24 of the sum of the absolute terms, the factor 2 is slack for the order
of the partial sums; bias and residual are two more additions; the last term is the stored result's rounding, twice over).

Three criteria per launch (Stats):
 (a) every element: r = |route - reference| / E <= 1;
 (b) every 16-frame x 16-output tile -- the kernel's tile, the last frame tile ragged: tile RMS of r <= encoder_ref.RHO x the
     launch's RMS of r.  A defect confined to one tile stands out against its own launch although each element stays under E;
 (c) level: the launch's RMS of r <= LEVEL x the RMS of r of `emulate` on the same input.  E is a worst case, thousands of
     times what a correct route uses, so a defect every element shares alike (one product missing everywhere) passes (a) and
     (b); against the emulation's level it does not.  LEVEL = 2 is for what the emulation does not model: the order of the
     four products inside one MFMA and whether they are fused.
RMS values are over the real columns (157 of a state's 192: the pad is exactly zero in route and reference alike).
"""
import torch

import encoder_ref as er

U_F32 = 2.0 ** -23
TILE = 16          # fc_rows16_f32's output tile: 16 frames x 16 outputs
LEVEL = 2.0        # criterion (c)
STATE = 192        # kStateStride
REAL = 157         # pose6d 144 | betas 10 | cam 3

# step -> (layer, step whose tap is the input (None = the features), step whose tap is the residual)
STEPS = {1: ("fc1x", None, None)}
for _i in range(3):
    STEPS[2 + 3 * _i] = ("fc1s", 4 + 3 * (_i - 1) if _i else 0, 1)
    STEPS[3 + 3 * _i] = ("fc2", 2 + 3 * _i, None)
    STEPS[4 + 3 * _i] = ("dec", 3 + 3 * _i, 4 + 3 * (_i - 1) if _i else 0)


class Layer:
    """One packed GEMM: w [N, K] and b [N] in float32 as uploaded (K, N padded), `real` = columns of the output that are
    not padding."""

    def __init__(self, w, b, real):
        self.w, self.b, self.real = w, b, real
        self.N, self.K = w.shape
        self.w64, self.b64 = w.double(), b.double()


def _t(a):
    return torch.as_tensor(a, dtype=torch.float32)


def layers(state_dict, device="cpu"):
    """The four GEMMs of a SPIN state dict as make_fc packs them -> {"fc1x", "fc1s", "fc2", "dec"}, and the initial state
    [192]."""
    sd = {(k[7:] if k.startswith("module.") else k): v for k, v in state_dict.items()}
    fc1w, fc1b = _t(sd["fc1.weight"]), _t(sd["fc1.bias"])
    assert fc1w.shape == (1024, 2048 + REAL)
    w1s = torch.zeros(1024, STATE)
    w1s[:, :REAL] = fc1w[:, 2048:]
    wd = torch.zeros(STATE, 1024)
    bd = torch.zeros(STATE)
    wd[:REAL] = torch.cat([_t(sd["decpose.weight"]), _t(sd["decshape.weight"]), _t(sd["deccam.weight"])])
    bd[:REAL] = torch.cat([_t(sd["decpose.bias"]), _t(sd["decshape.bias"]), _t(sd["deccam.bias"])])
    init = torch.zeros(STATE)
    init[:REAL] = torch.cat([_t(sd["init_pose"]).reshape(-1), _t(sd["init_shape"]).reshape(-1), _t(sd["init_cam"]).reshape(-1)])
    L = {"fc1x": Layer(fc1w[:, :2048].contiguous().to(device), fc1b.to(device), 1024),
         "fc1s": Layer(w1s.to(device), torch.zeros(1024, device=device), 1024),
         "fc2": Layer(_t(sd["fc2.weight"]).to(device), _t(sd["fc2.bias"]).to(device), 1024),
         "dec": Layer(wd.to(device), bd.to(device), REAL)}
    return L, init.to(device)


def reference(layer, a, res=None):
    """-> (z, E) of one launch in float64 from its float32 input a [M, K] and residual res [M, N] (or None)."""
    a = a.double()
    z = a @ layer.w64.T + layer.b64
    mag = a.abs() @ layer.w64.abs().T + layer.b64.abs()
    if res is not None:
        z = z + res.double()
        mag = mag + res.double().abs()
    return z, (layer.K + 2) * U_F32 * mag + U_F32 * z.abs()


def emulate(layer, a, res=None, skip=None):
    """The kernel's arithmetic in float32 on a's device: four ascending-k chains over the quarters of K (one per wave), every
    product rounded and every sum rounded, the four partial sums added in wave order, then the bias, then the residual.
    skip: a k whose product every element's chain leaves out (the checker's level defect)."""
    M = a.shape[0]
    kq = layer.K // 4
    a4 = a.float().reshape(M, 4, kq).permute(1, 0, 2).contiguous()              # [4, M, kq]
    w4 = layer.w.reshape(layer.N, 4, kq).permute(1, 0, 2).contiguous()          # [4, N, kq]
    acc = torch.zeros(4, M, layer.N, dtype=torch.float32, device=a.device)
    for k in range(kq):
        if skip is not None and k == skip % kq:
            keep = torch.ones(4, 1, 1, dtype=torch.float32, device=a.device)
            keep[skip // kq] = 0
        else:
            keep = None
        p = a4[:, :, k, None] * w4[:, None, :, k]
        acc = acc + (p if keep is None else p * keep)
    v = ((acc[0] + acc[1]) + acc[2]) + acc[3]
    v = v + layer.b
    if res is not None:
        v = v + res.float()
    return v


def ratios(got, ref, E):
    """r = |got - ref| / E elementwise (0 where the difference is 0, whatever E)."""
    return er.ratios(got.double(), ref, E)


def tile_rms(r, real):
    """RMS of r [M, N] over every 16-frame x 16-output tile, over the tile's real columns (< real) and the frames it has (the
    last frame tile may be ragged) -> [frame tiles, output tiles that hold a real column]."""
    M, N = r.shape
    nt = -(-real // TILE)
    q = (r[:, :real] ** 2)
    padm, padn = (-M) % TILE, nt * TILE - real
    q = torch.nn.functional.pad(q, (0, padn, 0, padm))
    s = q.reshape((M + padm) // TILE, TILE, nt, TILE).sum(dim=(1, 3))
    rows = torch.full(((M + padm) // TILE,), float(TILE), dtype=r.dtype, device=r.device)
    if padm:
        rows[-1] = TILE - padm
    cols = torch.full((nt,), float(TILE), dtype=r.dtype, device=r.device)
    if padn:
        cols[-1] = TILE - padn
    return (s / (rows[:, None] * cols[None, :])).sqrt()


class Stats:
    """Criteria (a) and (b) of one launch, and its RMS of r for (c)."""

    def __init__(self, got, ref, E, real):
        r = ratios(got, ref, E)
        self.max_r = float(r.max())
        self.rms = float((r[:, :real] ** 2).mean().sqrt())
        self.max_tile = float(tile_rms(r, real).max())
        self.pad_max = float(got[:, real:].abs().max()) if real < got.shape[1] else 0.0

    @property
    def tile_ratio(self):
        return self.max_tile / self.rms if self.rms > 0 else 0.0


def check(got, emu, ref, E, real):
    """-> (Stats of the route, Stats of the emulation, failures): failures lists which of (a), (b), (c) `got` misses."""
    s, e = Stats(got, ref, E, real), Stats(emu, ref, E, real)
    bad = []
    if not s.max_r <= 1.0:
        bad.append("a")
    if not s.tile_ratio <= er.RHO:
        bad.append("b")
    if not s.rms <= LEVEL * e.rms:
        bad.append("c")
    return s, e, bad
