"""Case tables, seeded input makers, float64 references and bars for the SchNet kernels at the ABI
(csrc/schnet.hip): the fused filter forward and backward, the W_1 gradient, the aggregation and the
ssp pair.  No GPU import: the CPU conditions are in test_schnet_cases_cpu.py, the GPU comparisons in
test_gpu_schnet_kernels.py.

Every reference is one function of (inputs, dtype): in float64 it is `ref`; with absolute=True it is
`den` (every product term by its absolute value, ssp replaced by softplus + ln 2, ssp' replaced by
1); in float32 on the CPU it is `r32`.  ssp' is replaced by 1 because the kernels take the derivative
from the OUTPUT, 1 - exp(-y) / 2 (include/mvml_gat.h): its absolute error is of order u = 2^-24, not
its relative error, so a den that followed ssp' towards 0 would reject the documented design.

Bars, all element-wise and unmasked (stat / fp32_check / allowed_check of _row_kernel_cases.py):

  bitwise: repeat runs, the zero_w rows, a zero dA row, empty lists (+0), a sub-range or a single
    list run alone, and exact inputs (integers times a per-row power of two, every partial sum below
    2^24 in the row's unit, so any order and any precision gives the float64 result; compared by
    value, so that the sign of a zero is not held).

  fp32 kernels (cfconv_agg, ssp_fwd, ssp_bwd, dpre2, dW_1):  |got - ref| <= max(4 e32, 8 u) den,
    e32 the statistic of the float32 CPU run of the same formulas (fp32_check).

  split-fp16 products, the GEMM tests' rule  B(e_cpu) = 3 * 2^-22 + 4 e_cpu  on den of the product:
    s1 = ssp(pre1), pre1 = rbf W_1^T + b_1.  The kernel's pre1 is within B(e1) den(pre1); e1 is the
      statistic of the float32 CPU evaluation of pre1 INCLUDING its float32 exp(-gamma (d - mu)^2)
      against float64 on the same inputs (the device expf has no stated error: it is measured the
      way e_cpu is, and the factor 4 is the standing margin for another valid fp32 evaluation).
      ssp is 1-Lipschitz, and evaluating it in fp32 costs at most the fp32 ssp bar S1 = max(4 e32, 8 u)
      (e32 of ssp on these pre-activations) on its own den:
          allowed(s1) = B(e1) den(pre1) + S1 den(s1)
    he = ssp(pre2), pre2 = s1 W_2^T + b_2 on the kernel's own s1, which is within allowed(s1):
          allowed(he) = B(e2) ((|s1| + allowed(s1)) |W_2|^T + |b_2|) + allowed(s1) |W_2|^T + S2 den(he)
      e2 the fp32 CPU product of the fp32-rounded reference s1.
    dpre1 = (dpre2 W_2) ssp'(s1) on the kernel's own dpre2, within its fp32 bar D2 den(dpre2):
          allowed(dpre1) = B(eB) P + (D2 den(dpre2)) |W_2| + G P,   P = den(dpre2) |W_2|
      G the fp32 bar of ssp' measured absolutely (den 1) on the given s1.
  e1, e2 and eB are taken with 2^-126 (the smallest normal fp32) off the difference, and 2^-126 is
  added to the allowance, as _row_kernel_cases.py does: a pre-activation made of rbf terms far below
  2^-126 is flushed to 0 by the device and by the CPU alike, which is an error of 1 relative to a den
  of 1e-48 and would otherwise swamp the whole case's bar.
  The backward's s1 and he are INPUTS: the float32 roundings of the reference, as the LayerNorm
  backward is given mean and rstd.
"""
import ctypes
import math
import zlib
from dataclasses import dataclass

import torch
import torch.nn.functional as F

import _schnet_ref as SR
from _gemm_cases import BAR_SPLIT, amax_shift, emulate_split
from _row_kernel_cases import TINY, U, allowed_check, fp32_bar, fp32_check, stat  # noqa: F401 (re-exported)

F64, F32 = torch.float64, torch.float32
LN2 = math.log(2.0)
# csrc/schnet.hip: kSnTile, kSnWgE, kSnMaxSplits, kSnMaxK, kSnMaxH, kSnRbfShift
TILE, WG_E, MAX_SPLITS, MAX_K, MAX_H, RBF_SHIFT = 128, 32, 128, 512, 128, 14
SSP_GRID_CAP = 8192 * 256


def _gen(name):
    return torch.Generator().manual_seed(zlib.crc32(name.encode()))


def _randn(g, *shape):
    return torch.randn(shape, generator=g)


def _ints(g, *shape):
    return torch.randint(-8, 9, shape, generator=g).float()


# ====================================================================== the source, restated
def instance(H):
    """by_width: the NTB of the filter kernels' instance."""
    return 2 if H <= 32 else 4 if H <= 64 else 8


def agg_instance(H):
    """mvml_cfconv_agg: lanes per atom."""
    return 16 if H <= 64 else 64


def sn_ks(K):
    return (K + 31) // 32


def image_bytes(H, K):
    """[256 B header][W_1: ks(K) x H/16 blocks][W_2][W_2^T: ks(H) x H/16 blocks], 128 x 16 B a block."""
    return 256 + 16 * (sn_ks(K) * (H // 16) * 128 + 2 * sn_ks(H) * (H // 16) * 128)


def dw1_splits(E):
    return max(1, min(-(-E // (4 * WG_E)), MAX_SPLITS))


def dw1_per(E):
    return -(-(-(-E // WG_E)) // dw1_splits(E)) * WG_E


def dw1_empty_ranges(E):
    return sum(1 for x in range(dw1_splits(E)) if x * dw1_per(E) >= E)


def dw1_workspace(E, H, K):
    return ((dw1_splits(E) * H * K * 4 + 255) & ~255) + 256


# ====================================================================== the filter
F_E = (1, 15, 16, 17, 31, 32, 33, 127, 128, 129, 255, 256, 257, 385)
F_H = (16, 32, 48, 64, 80, 96, 112, 128)
F_K = (1, 8, 31, 32, 33, 63, 64, 65, 300, 511, 512)
F_EDGES = (1, 33, 128, 129)            # with every instance
PADS = (0, 4, 12)
NODES = 23                             # atoms of a filter case's graph (21 row scales, a zero row, one more)
ZERO_ROW = 5
# (H, K, E): every instance with every E edge first, then the rest of each axis
F_TRIPLES = ((16, 1, 1), (32, 31, 33), (16, 32, 128), (32, 33, 129),
             (48, 63, 1), (64, 64, 33), (48, 65, 128), (64, 8, 129),
             (80, 511, 1), (128, 512, 33), (96, 8, 128), (112, 1, 129),
             (16, 8, 15), (32, 64, 16), (48, 32, 17), (64, 33, 31), (80, 31, 32), (96, 65, 127),
             (112, 63, 255), (128, 8, 256), (80, 64, 257), (64, 300, 385), (128, 300, 385), (32, 512, 385))
REGIMES = ("normal", "rows", "zero_w1", "zero_w2", "saturated", "onehot")


@dataclass(frozen=True)
class FC:
    H: int
    K: int
    E: int
    ldd: int
    pads: tuple                        # pitch - H of (s1, he, dA, hv, dpre2, dpre1)

    @property
    def name(self):
        return f"filter/h{self.H}k{self.K}e{self.E}/d{self.ldd}/p{'.'.join(map(str, self.pads))}"

    @property
    def ntb(self):
        return instance(self.H)

    def ld(self, i):
        return self.H + self.pads[i]


F_CASES = tuple(FC(h, k, e, 1 + 2 * (i % 2), tuple(PADS[(i + j + j // 3) % 3] for j in range(6)))
                for i, (h, k, e) in enumerate(F_TRIPLES))


def regime_cases(regime):
    """normal: the whole table.  onehot: every case with E >= K (each centre is hit).  The others:
    per instance its first and last width at a partial tile, and the one-slot cases."""
    if regime == "normal":
        return F_CASES
    if regime == "onehot":
        return tuple(c for c in F_CASES if c.E >= c.K)
    return tuple(c for c in F_CASES if (c.H, c.E) in ((16, 1), (32, 129), (48, 1), (64, 385), (80, 257), (128, 33),
                                                      (112, 255), (96, 127), (16, 15), (32, 16)))


def centers_of(K, gap):
    """RBFExpansion's grid: arange(0, K) * gap."""
    return torch.arange(K, dtype=F32) * gap


def filter_inputs(c, regime):
    """d [E], centers [K], gamma, W_1 [H][K], b_1, W_2 [H][H], b_2 and the backward's graph on NODES
    atoms: in_src / slot_dst [E] (int32), hv and dA [NODES][H]."""
    g = _gen(c.name + regime)
    E, H, K = c.E, c.H, c.K
    if regime == "onehot":
        gap, gamma = 0.5, 440.0                             # gamma gap^2 = 110: every off-centre term is 0
        cen = centers_of(K, gap)
        d = cen[torch.arange(E) % K].clone()
        W1, b1, W2, b2 = _ints(g, H, K) / 8, _ints(g, H) / 8, _ints(g, H, H) / 8, _ints(g, H) / 8
    else:
        gap, gamma = 0.1, 10.0
        cen = centers_of(K, gap)
        cutoff = K * gap
        d = torch.rand(E, generator=g) * 1.1 * cutoff
        d[0] = 0.0
        if E > 1:
            d[1] = cen[K // 2]
        if E > 2:
            d[2] = 10.0 * cutoff                            # rbf all zero or subnormal
        W1, b1, W2, b2 = _randn(g, H, K) / K ** 0.5, _randn(g, H), _randn(g, H, H) / H ** 0.5, _randn(g, H)
    if regime == "zero_w1":
        W1 = torch.zeros(H, K)
    elif regime == "zero_w2":
        W2 = torch.zeros(H, H)
    elif regime == "saturated":
        lv = torch.tensor([-30.0, -8.0, 0.0, 8.0, 30.0])
        b1, b2 = lv[torch.arange(H) % 5], lv[(torch.arange(H) // 5 + torch.arange(H)) % 5]
    src = torch.randint(0, NODES, (E,), generator=g, dtype=torch.int32)
    dst = torch.randint(0, NODES, (E,), generator=g, dtype=torch.int32)
    hv, dA = _randn(g, NODES, H), _randn(g, NODES, H)
    if regime == "rows":
        e = torch.pow(2.0, -(torch.arange(NODES) % 21).float())[:, None]
        hv, dA = hv * e, dA * e.flip(0).roll(3, 0)
        dA[ZERO_ROW] = 0.0
        dst[E - 1] = ZERO_ROW
        if E > 3:
            src[E - 2], dst[E - 2] = 20, 22                 # 2^-20 * 2^-20: the smallest row next to the largest
            src[E - 3], dst[E - 3] = 0, 2
    return {"d": d, "centers": cen, "gamma": gamma, "W1": W1, "b1": b1, "W2": W2, "b2": b2, "src": src, "dst": dst,
            "hv": hv, "dA": dA}


def _sp(x):
    return F.softplus(x) + LN2


def sspg(y):
    """ssp' from the output."""
    return 1.0 - 0.5 * torch.exp(-y)


def rbf_of(inp, dt=F64):
    return torch.exp(-inp["gamma"] * (inp["d"].to(dt)[:, None] - inp["centers"].to(dt)[None, :]) ** 2)


def filter_fwd(inp, dt=F64, absolute=False):
    """{rbf, pre1, s1, pre2, he}; s1 and he are what _schnet_ref.filter computes."""
    W1, b1, W2, b2 = (inp[k].to(dt) for k in ("W1", "b1", "W2", "b2"))
    rbf = rbf_of(inp, dt)
    if absolute:
        p1 = rbf @ W1.abs().T + b1.abs()
        s1 = _sp(p1)
        p2 = s1 @ W2.abs().T + b2.abs()
        return {"rbf": rbf, "pre1": p1, "s1": s1, "pre2": p2, "he": _sp(p2)}
    p1 = F.linear(rbf, W1, b1)
    s1 = SR.ssp(p1)
    p2 = F.linear(s1, W2, b2)
    return {"rbf": rbf, "pre1": p1, "s1": s1, "pre2": p2, "he": SR.ssp(p2)}


def ssp_bar(x32):
    """The fp32 bar of ssp on the fp32 pre-activations x32."""
    return fp32_bar(stat(SR.ssp(x32), SR.ssp(x32.double()), _sp(x32.double().abs())))


def sspg_bar(y32):
    """The fp32 bar of ssp' on the fp32 outputs y32, absolute (den 1)."""
    return fp32_bar(stat(sspg(y32), sspg(y32.double()), torch.ones_like(y32, dtype=F64)))


def fwd_bars(inp):
    """(ref, den, {"s1": allowed, "he": allowed}, {the measured pieces}) -- the module docstring."""
    r, a, r32 = filter_fwd(inp), filter_fwd(inp, absolute=True), filter_fwd(inp, F32)
    W2a, b2 = inp["W2"].double().abs(), inp["b2"].double()
    e1 = stat(r32["pre1"], r["pre1"], a["pre1"], TINY)
    S1, S2 = ssp_bar(r["pre1"].float()), ssp_bar(r["pre2"].float())
    al_s1 = (BAR_SPLIT + 4 * e1) * a["pre1"] + S1 * a["s1"] + TINY
    s1in = r["s1"].float()
    den2 = s1in.double().abs() @ W2a.T + b2.abs()
    e2 = stat(F.linear(s1in, inp["W2"], inp["b2"]), F.linear(s1in.double(), inp["W2"].double(), b2), den2, TINY)
    al_he = (BAR_SPLIT + 4 * e2) * ((s1in.double().abs() + al_s1) @ W2a.T + b2.abs()) + al_s1 @ W2a.T + S2 * a["he"]
    return r, a, {"s1": al_s1, "he": al_he}, {"e1": e1, "e2": e2, "S1": S1, "S2": S2}


def bwd_given(inp):
    """The backward's s1 and he inputs: the reference rounded to fp32."""
    r = filter_fwd(inp)
    return r["s1"].float(), r["he"].float()


def filter_bwd(inp, s1, he, dt=F64, absolute=False):
    """(dpre2, dpre1) [E][H] from the given s1 and he."""
    g, h = inp["dA"].to(dt)[inp["dst"].long()], inp["hv"].to(dt)[inp["src"].long()]
    W2 = inp["W2"].to(dt)
    if absolute:
        dp2 = g.abs() * h.abs()
        return dp2, dp2 @ W2.abs()
    dp2 = (g * h) * sspg(he.to(dt))
    return dp2, (dp2 @ W2) * sspg(s1.to(dt))


def bwd_bars(inp, s1, he):
    """(ref pair, den pair, r32 of dpre2, allowed(dpre1), pieces)."""
    r, a, r32 = filter_bwd(inp, s1, he), filter_bwd(inp, s1, he, absolute=True), filter_bwd(inp, s1, he, F32)
    D2 = fp32_bar(stat(r32[0], r[0], a[0]))
    W2 = inp["W2"]
    dp2in = r[0].float()
    denB = dp2in.double().abs() @ W2.double().abs()
    eB = stat(dp2in @ W2, dp2in.double() @ W2.double(), denB, TINY)
    G = sspg_bar(s1)
    allowed = (BAR_SPLIT + 4 * eB) * a[1] + (D2 * a[0]) @ W2.double().abs() + G * a[1] + TINY
    return r, a, r32[0], allowed, {"D2": D2, "eB": eB, "G": G}


# ---------------------------------------------------------------------- exact2: W_2^T's image, bitwise
EXACT_Y = 30.0                          # ssp'(30) = 1 - exp(-30) / 2 rounds to exactly 1 in fp32


def exact2_inputs(c):
    """Hand-made backward operands: s1 = he = 30 everywhere (ssp' is exactly 1: the CPU test proves it
    for any expf within a factor of two), dA and hv integers in [-8, 8] times 2^-e per row, e <= 10
    each, W_2 integers / 8.  dpre2 = dA[dst] hv[src] and dpre1 = dpre2 W_2 are then exact in any order:
    integers below 2^6 resp. 128 * 2^6 * 2^3 = 2^16 in the row's unit."""
    g = _gen(c.name + "exact2")
    e = torch.pow(2.0, -(torch.arange(NODES) % 11).float())[:, None]
    inp = {"W2": _ints(g, c.H, c.H) / 8, "hv": _ints(g, NODES, c.H) * e, "dA": _ints(g, NODES, c.H) * e.flip(0),
           "src": torch.randint(0, NODES, (c.E,), generator=g, dtype=torch.int32),
           "dst": torch.randint(0, NODES, (c.E,), generator=g, dtype=torch.int32),
           "W1": torch.zeros(c.H, c.K)}
    inp["dA"][ZERO_ROW] = 0.0
    inp["dst"][c.E - 1] = ZERO_ROW
    y = torch.full((c.E, c.H), EXACT_Y)
    return inp, y, y.clone()


def exact2_expected(inp):
    g, h = inp["dA"].double()[inp["dst"].long()], inp["hv"].double()[inp["src"].long()]
    return (g * h).float(), ((g * h) @ inp["W2"].double()).float()


# ---------------------------------------------------------------------- the split path on the CPU
def emulate_fwd(inp, drop2=False, global_scale=False, swap_w1=None):
    """schnet_filter_fwd_kernel's arithmetic with _gemm_cases.emulate_split: rbf at the fixed 2^14 times
    W_1 at its operand-wide scale, ssp in fp32, s1 re-split per row, times W_2.  Mutations: drop2 leaves
    l_a h_b out of product 2; global_scale gives s1 one scale; swap_w1 = (k, k') exchanges two W_1
    columns.  (s1, he) in fp32."""
    W1 = inp["W1"].clone()
    if swap_w1:
        k, k2 = swap_w1
        W1[:, [k, k2]] = W1[:, [k2, k]]
    rbf = rbf_of(inp, F32)
    sa = torch.full((rbf.shape[0], 1), RBF_SHIFT, dtype=torch.int32)
    p1 = emulate_split(rbf, W1, sa, amax_shift(W1.abs().max())).float() + inp["b1"]
    s1 = SR.ssp(p1)
    row = s1.abs().amax(1, keepdim=True)
    ss = amax_shift(row.max()).expand(s1.shape[0], 1) if global_scale else amax_shift(row)
    p2 = emulate_split(s1, inp["W2"], ss, amax_shift(inp["W2"].abs().max()), drop=drop2).float() + inp["b2"]
    return s1, SR.ssp(p2)


def emulate_bwd(inp, s1, he, drop=False, global_scale=False):
    """schnet_filter_bwd_kernel: dpre2 in fp32, split per row, times W_2^T's image.  (dpre2, dpre1)."""
    dp2 = filter_bwd(inp, s1, he, F32)[0]
    row = dp2.abs().amax(1, keepdim=True)
    ss = amax_shift(row.max()).expand(dp2.shape[0], 1) if global_scale else amax_shift(row)
    ds1 = emulate_split(dp2, inp["W2"].T.contiguous(), ss, amax_shift(inp["W2"].abs().max()), drop=drop).float()
    return dp2, ds1 * sspg(s1)


# ====================================================================== dW_1
D_K = (1, 15, 16, 17, 63, 64, 65, 512)
D_BIG = (16384, 16385, 16417)


@dataclass(frozen=True)
class DC:
    H: int
    K: int
    E: int
    accumulate: int
    ldd: int
    pad: int

    @property
    def name(self):
        return f"dw1/h{self.H}k{self.K}e{self.E}/a{self.accumulate}d{self.ldd}p{self.pad}"


D_CASES = tuple([DC(F_H[(3 * i) % 8], D_K[i % 8], e, i % 2, 1 + 2 * ((i // 2) % 2), PADS[i % 3]) for i, e in enumerate(F_E)]
                + [DC(16, k, e, (i + j) % 2, 1 + 2 * j, PADS[(i + j) % 3]) for i, e in enumerate(D_BIG)
                   for j, k in enumerate((1, 65))]
                + [DC(128, 512, 129, 1, 1, 4), DC(80, 65, 257, 0, 3, 12)])


def dw1_inputs(c):
    g = _gen(c.name)
    gap = 0.1
    d = torch.rand(c.E, generator=g) * 1.1 * c.K * gap
    d[0] = 0.0
    return {"d": d, "centers": centers_of(c.K, gap), "gamma": 10.0, "dpre1": _randn(g, c.E, c.H),
            "base": _randn(g, c.H, c.K)}


def dw1_eval(c, inp, dt=F64, absolute=False, leave_out_last=False):
    """dW_1 [H][K] (+ base when the case accumulates)."""
    rbf, g, base = rbf_of(inp, dt), inp["dpre1"].to(dt), inp["base"].to(dt)
    if leave_out_last:
        rbf, g = rbf[:-1], g[:-1]
    if absolute:
        g, base = g.abs(), base.abs()
    out = g.T @ rbf
    return out + base if c.accumulate else out


# ====================================================================== the aggregation
A_DEGS = (0, 1, 15, 16, 17, 63, 64, 65, 129)
A_N = (1, 3, 4, 5, 15, 16, 17, 63, 64, 65)
A_H = (16, 64, 80, 128)
A_DIRS = ("in", "out")                 # widx NULL (a) | widx a permutation (dL/dhv)


@dataclass(frozen=True)
class AC:
    N: int
    H: int
    direction: str
    rot: int
    pads: tuple                        # (X, Wt, out)

    @property
    def name(self):
        return f"agg/n{self.N}h{self.H}/{self.direction}/r{self.rot}p{'.'.join(map(str, self.pads))}"

    @property
    def degrees(self):
        """From A_DEGS, rotated; N >= 2: a 129-list and an empty list side by side in atoms 0, 1 (one
        wave's four-atom group at H <= 64); N = 1: 17, 65 or 129."""
        if self.N == 1:
            return [(17, 65, 129)[self.rot % 3]]
        dg = [A_DEGS[(i * 4 + self.rot) % 9] for i in range(self.N)]
        dg[0], dg[1] = 129, 0
        return dg


A_CASES = tuple(AC(n, A_H[(i + j) % 4], dr, i + 2 * j, tuple(PADS[(i + j + t) % 3] for t in range(3)))
                for j, dr in enumerate(A_DIRS) for i, n in enumerate(A_N)) + \
    (AC(1, 64, "in", 1, (0, 4, 12)), AC(1, 128, "out", 2, (4, 0, 0)), AC(1, 80, "in", 0, (12, 4, 0)))


def agg_inputs(c, exact=False):
    """rowptr [N + 1], widx [E] | None, xidx [E] (int32, written out: the kernel sees nothing else),
    X [N + 2][H], Wt [E][H].  xidx repeats and reaches the last row of X.  exact: X integers, Wt
    integers times 2^-(v % 21) of the list v that owns the entry: 129 * 64 < 2^14 units."""
    g = _gen(c.name + ("exact" if exact else ""))
    dg = c.degrees
    rowptr = torch.tensor([0] + list(torch.tensor(dg).cumsum(0)), dtype=torch.int32)
    E, NX = int(rowptr[-1]), c.N + 2
    xidx = torch.randint(0, NX, (E,), generator=g, dtype=torch.int32)
    xidx[0], xidx[E - 1] = NX - 1, xidx[E // 2]
    widx = torch.randperm(E, generator=g).to(torch.int32) if c.direction == "out" else None
    owner = torch.repeat_interleave(torch.arange(c.N), torch.tensor(dg))
    if exact:
        X, Wt = _ints(g, NX, c.H), _ints(g, E, c.H)
        w = torch.arange(E) if widx is None else widx.long()
        Wt[w] = Wt[w] * torch.pow(2.0, -(owner % 21).float())[:, None]
    else:
        X, Wt = _randn(g, NX, c.H), _randn(g, E, c.H)
    return {"rowptr": rowptr, "widx": widx, "xidx": xidx, "X": X, "Wt": Wt, "owner": owner, "E": E}


def agg_eval(c, inp, dt=F64, absolute=False, leave_out_last_of=()):
    """out [N][H]; leave_out_last_of: degrees whose lists lose their last entry (a mutation)."""
    w = torch.arange(inp["E"]) if inp["widx"] is None else inp["widx"].long()
    X, Wt = inp["X"].to(dt), inp["Wt"].to(dt)
    if absolute:
        X, Wt = X.abs(), Wt.abs()
    terms = X[inp["xidx"].long()[w]] * Wt[w]
    keep = torch.ones(inp["E"], dtype=torch.bool)
    for v, n in enumerate(c.degrees):
        if n in leave_out_last_of:
            keep[int(inp["rowptr"][v + 1]) - 1] = False
    return torch.zeros((c.N, c.H), dtype=dt).index_add_(0, inp["owner"][keep], terms[keep])


# ====================================================================== ssp
S_N = (1, 255, 256, 257, SSP_GRID_CAP + 1)
# (89: the first planted value whose fp32 exp overflows; exp(88) = 1.65e38 is still finite)
S_PLANTED = (0.0, 2.0 ** -30, -2.0 ** -30, 1.0, -1.0, 19.999, 20.0, 20.001, 88.0, 89.0, -20.0, -104.0)


@dataclass(frozen=True)
class SC:
    n: int
    inplace: bool

    @property
    def name(self):
        return f"ssp/{self.n}/{'in' if self.inplace else 'out'}place"


S_CASES = tuple(SC(n, ip) for n in S_N[:4] for ip in (False, True)) + (SC(S_N[4], True),)


def ssp_inputs(c):
    g = _gen(c.name)
    x = 6.0 * _randn(g, c.n)
    pl = torch.tensor(S_PLANTED, dtype=F32)
    if c.n == 1:
        x[0] = 88.0
    else:
        for base in (3, c.n - len(pl)):                     # near the start and in the last block / sweep
            x[base:base + len(pl)] = pl
    return {"x": x, "y": SR.ssp(x), "gy": _randn(g, c.n)}


def ssp_fwd(inp, dt=F64, absolute=False, threshold=True):
    x = inp["x"].to(dt)
    if absolute:
        return _sp(x.abs())
    return SR.ssp(x) if threshold else torch.log1p(torch.exp(x)) - LN2


def ssp_bwd(inp, dt=F64, absolute=False):
    """g_x from the GIVEN fp32 y."""
    gy = inp["gy"].to(dt)
    return gy.abs() if absolute else gy * sspg(inp["y"].to(dt))


# ====================================================================== the refusals
INVALID, WORKSPACE = 1, 3
RH, RK, RE = 16, 8, 4
# per entry: who, argument names, and which argument is what
SPEC = {
    "mvml_schnet_split_w": dict(who="schnet_split_w", args="H K W1 W2 image stream", ptrs="W1 W2 image", al="image"),
    "mvml_schnet_filter_fwd": dict(who="schnet_filter_fwd", args="E d ldd centers K gamma H image b1 b2 s1 lds1 he ldhe stream",
                                   ptrs="d centers image b1 b2 s1 he", al="image", mats="s1:lds1 he:ldhe"),
    "mvml_schnet_filter_bwd": dict(who="schnet_filter_bwd",
                                   args="E in_src slot_dst dA lda hv ldh s1 lds1 he ldhe H K image dpre2 ld2 dpre1 ld1 stream",
                                   ptrs="in_src slot_dst dA hv s1 he image dpre2 dpre1", al="image",
                                   mats="dA:lda hv:ldh s1:lds1 he:ldhe dpre2:ld2 dpre1:ld1"),
    "mvml_schnet_dw1": dict(who="schnet_dw1", args="E d ldd centers K gamma dpre1 ld1 H accumulate dW1 workspace workspace_bytes stream",
                            ptrs="d centers dpre1 dW1", mats="dpre1:ld1"),
    "mvml_cfconv_agg": dict(who="cfconv_agg", args="N E rowptr widx xidx X ldx Wt ldw H out ldo stream",
                            ptrs="rowptr xidx X Wt out", mats="X:ldx Wt:ldw out:ldo"),
    "mvml_ssp_fwd": dict(who="ssp_fwd", args="n x y stream", ptrs="x y"),
    "mvml_ssp_bwd": dict(who="ssp_bwd", args="n y g_y g_x stream", ptrs="y g_y g_x"),
}


def _good(entry, P):
    ws = dw1_workspace(RE, RH, RK)
    v = dict(H=RH, K=RK, E=RE, N=3, n=5, ldd=1, gamma=10.0, accumulate=0, workspace_bytes=ws, stream=None)
    out = []
    for a in SPEC[entry]["args"].split():
        out.append(v[a] if a in v else RH if a.startswith("ld") else P)
    return out


def refusals(P, P_off):
    """{id: (entry, the word mvml_last_error() must hold, code, args)}: every documented refusal of the
    SchNet entries.  P stands for every pointer (16-byte aligned, P_off 4 bytes past it); the last
    argument is the stream."""
    out = {}
    for entry, sp in SPEC.items():
        names = sp["args"].split()

        def put(what, arg, value, code=INVALID):
            a = _good(entry, P)
            a[names.index(arg)] = value
            out[f"{entry}:{what}"] = (entry, sp["who"], code, a)

        for p in sp["ptrs"].split():
            put(p + " NULL", p, None)
        for p in sp.get("al", "").split() + [m.split(":")[0] for m in sp.get("mats", "").split()]:
            put(p + " misaligned", p, P_off)
        for m in sp.get("mats", "").split():
            ld = m.split(":")[1]
            put(f"{ld}=H-4", ld, RH - 4)
            put(f"{ld}=H+2", ld, RH + 2)
        if "ldd" in names:
            put("ldd=0", "ldd", 0)
        if "gamma" in names:
            for gv in (0.0, -1.0, float("inf"), float("nan")):
                put(f"gamma={gv}", "gamma", gv)
        if "E" in names:
            put("E=-1", "E", -1)
            put("E=2^31-128", "E", 2 ** 31 - 128)
        if "N" in names:
            put("N=-1", "N", -1)
        if "n" in names:
            put("n=-1", "n", -1)
        if "workspace" in names:
            put("workspace NULL", "workspace", None, WORKSPACE)
            put("workspace short", "workspace_bytes", dw1_workspace(RE, RH, RK) - 1, WORKSPACE)
    return out


def violations(entry, args):
    """The documented conditions of include/mvml_gat.h that an argument list breaks, restated."""
    sp = SPEC[entry]
    a = dict(zip(sp["args"].split(), args))
    val = lambda p: p.value if isinstance(p, ctypes.c_void_p) else p        # noqa: E731
    bad = []
    if "H" in a and not (16 <= a["H"] <= MAX_H and a["H"] % 16 == 0):
        bad.append("H")
    if "K" in a and not 1 <= a["K"] <= MAX_K:
        bad.append("K")
    if "E" in a and not 0 <= a["E"] < 2 ** 31 - TILE:
        bad.append("E")
    if "N" in a and not 0 <= a["N"] < 2 ** 31:
        bad.append("N")
    if "n" in a and a["n"] < 0:
        bad.append("n")
    if "gamma" in a and not (0.0 < a["gamma"] <= 3.0e38):
        bad.append("gamma")
    if "ldd" in a and a["ldd"] < 1:
        bad.append("ldd")
    for p in sp["ptrs"].split():
        if not val(a[p]):
            bad.append(p + " NULL")
    for p in sp.get("al", "").split() + [m.split(":")[0] for m in sp.get("mats", "").split()]:
        if val(a[p]) and val(a[p]) % 16:
            bad.append(p + " misaligned")
    for m in sp.get("mats", "").split():
        ld = a[m.split(":")[1]]
        if ld % 4 or ld < a["H"]:
            bad.append(m + " pitch")
    if "workspace" in a:
        if not val(a["workspace"]):
            bad.append("workspace NULL")
        elif "E" not in bad and a["workspace_bytes"] < dw1_workspace(a["E"], a["H"], a["K"]):   # (no size for a bad E)
            bad.append("workspace short")
    return bad
