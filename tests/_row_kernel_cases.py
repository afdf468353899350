"""Case tables, seeded input makers, float64 references and bars for the small kernels every training
step runs, at the ABI: GraphNorm and the ReLU backward (csrc/norm.hip), LayerNorm rows, plain token
attention and BCE-with-logits (csrc/fusion_attn.hip), mvml_add_cols_f32 (csrc/gatv2_agg.hip) and the
optimizer pair (csrc/optim.hip).  No GPU import: the CPU conditions are in
test_row_kernel_cases_cpu.py, the GPU comparisons in test_gpu_row_kernels.py (the optimizer pair
included: the whole file runs in a few seconds).

Every reference is one function of (inputs, dtype): in float64 it is the reference (`ref`), with
absolute values in place of every term it is `den`, and in float32 on the CPU it is `r32`, the
yardstick of what fp32 arithmetic itself loses on the case's inputs.

Bars (u = 2^-24):

  relu_bwd, add_cols, grad_gather, a skipped Adam parameter, repeat runs of everything: bitwise.

  GraphNorm (fp64 inside, one rounding to fp32 at the store):
      |got - ref| <= 2^-23 |ref| + 2 (n + G + 8) 2^-53 den
    The first term is the final fp32 rounding (2^-24 |ref|) with one more ulp for double rounding.
    The second: a column of a group of n rows is a sum of n terms (n - 1 adds), then at most 8 more
    fp64 operations per element (divide, multiply by mean_scale, subtract, square root, divide,
    multiply, add; the backward's k1, k2 products), each within 2^-53 of den; the parameter
    gradients add the G group partials (G more adds; n is then the longest group).  Doubled.
    fp32 statistics on x + 1000 would be 2^-24 * 1000 / std off: ten thousand times this bar.

  LayerNorm, token attention, BCE, Adam (fp32 kernels):
      |got - ref| <= bar * den,   bar = max(4 e32, 8 u),   e32 = max |r32 - ref| / den
    over the case's own inputs.  Their operation counts (below) all contain a device sqrtf, expf,
    log1pf or a division, whose error is neither derivable here nor stated in a document shipped
    with the toolchain, so the bar is measured: a correct fp32 kernel differs from the fp32 CPU
    run by reduction order and libm only, which four times its error covers, and 8 u is the floor
    where the CPU run happens to be exact.
      layernorm_fwd: 8 slot adds + 6 wave-reduction adds + 1 divide per statistic, twice, sqrtf, a
        divide, then subtract, 2 multiplies and an add per element: depth 14 per sum.
      layernorm_bwd: 2 ops per element before two sums of depth 14, then 4 ops per element.
      token_attn_fwd: kV <= 6 fmas + 6 reduction adds per score, a multiply, expf, 2 adds, a divide,
        3 fmas per output.  A score error d_j moves P_i by P_i (d_i - sum_j P_j d_j), so
        den(P_i) = P_i (1 + sA_i + sum_j P_j sA_j), sA the score's den, and den(att) follows.
      token_attn_bwd: 12 per dot product, 3 for `dot`, 3 per g_s, 3 fmas per output.  P is an INPUT
        here (the fp32 values given), so the reference has no softmax.
      bce_logits: fmaxf, multiply, subtract, expf, log1pf, add; expf, add, divide, subtract, divide.
      adam_flat: at most 16 fp32 operations per element, one sqrtf and two divides among them.
    Next to this bar, stated as the formula above, the same comparison is made once more with
    2^-126 (the smallest normal fp32) subtracted from both |got - ref| and |r32 - ref| first: a
    planted logit of -89 or a saturated softmax has results far below 2^-126, which both a
    correct kernel and the CPU flush to 0, so that e32 = 1 and the first bar holds nothing for the
    rest of that case; the second one is not swamped and is the one that binds there.
"""
import math
import zlib
from dataclasses import dataclass

import torch

U = 2.0 ** -24
TINY = 2.0 ** -126
F64, F32 = torch.float64, torch.float32
EPS32 = float(torch.tensor(1e-5, dtype=F32))          # (double)1e-5f: what the ABI receives


def _gen(name):
    return torch.Generator().manual_seed(zlib.crc32(name.encode()))


def _randn(g, *shape):
    return torch.randn(shape, generator=g)


def fp32_bar(e32):
    return max(4.0 * e32, 8.0 * U)


def stat(x, ref, den, floor=0.0):
    """max over elements of max(|x - ref| - floor, 0) / den (inf where den == 0 and it is not 0)."""
    d = ((x.double() - ref).abs() - floor).clamp_min(0.0)
    d = torch.nan_to_num(d, nan=float("inf"))
    ok = den > 0
    if bool((d[~ok] != 0).any()):
        return float("inf")
    return (d[ok] / den[ok]).max().item() if bool(ok.any()) else 0.0


def fp32_check(got, ref, den, r32):
    """The fp32 kernels' comparison: (record, ok).  e against max(4 e32, 8 u), and the same with
    2^-126 taken off both differences first (the module docstring)."""
    e, e32 = stat(got, ref, den), stat(r32, ref, den)
    ef, e32f = stat(got, ref, den, TINY), stat(r32, ref, den, TINY)
    rec = {"e": e, "bar": fp32_bar(e32), "ratio": e / fp32_bar(e32), "e_floor": ef, "bar_floor": fp32_bar(e32f),
           "ratio_floor": ef / fp32_bar(e32f)}
    return rec, e <= rec["bar"] and ef <= rec["bar_floor"]


def allowed_check(got, ref, allowed):
    """An element-wise allowance (GraphNorm): (record of the worst element, ok)."""
    d = torch.nan_to_num((got.double() - ref).abs(), nan=float("inf"))
    r = torch.where(allowed > 0, d / allowed.clamp_min(1e-300), torch.where(d == 0, 0.0, float("inf")).double())
    if r.numel() == 0:
        return {"e": 0.0, "bar": 0.0, "ratio": 0.0}, True
    i = int(r.reshape(-1).argmax())
    rec = {"e": float(d.reshape(-1)[i]), "bar": float(allowed.reshape(-1)[i]), "ratio": float(r.reshape(-1)[i])}
    return rec, rec["ratio"] <= 1.0


# ====================================================================== GraphNorm
GN_D = (1, 15, 16, 17, 255, 256, 257, 768)
GN_G = (1, 2, 16, 17, 48, 49, 63, 64, 65, 113, 129)
GN_SIZES = (0, 1, 2, 3, 64, 130)
# (x pattern, mean_scale pattern)
GN_PATTERNS = (("normal", "rand"), ("offset", "one"), ("const", "one"), ("normal", "zero"), ("offset", "rand"))
GN_PAIRS = ((1, 1), (2, 15), (16, 16), (17, 17), (48, 255), (49, 257), (63, 15), (64, 17), (65, 256), (113, 255),
            (129, 768), (129, 17), (1, 768), (64, 257))
GN_ALL_PATTERNS_AT = ((2, 15), (49, 257), (64, 17), (129, 768), (113, 255))


def gn_regime(G):
    """graphnorm_param_reduce: stripe s walks g = s, s + 64, .. while g + 48 < G (unrolled by 4), then
    a tail.  tail: no stripe enters the body; partial: stripe 0 does, stripe 15 does not; all: every
    stripe does, once; two: stripe 0 makes two trips."""
    trips = lambda s: len([g for g in range(s, G, 64) if g + 48 < G])   # noqa: E731
    if trips(0) == 0:
        return "tail"
    if trips(0) >= 2:
        return "two"
    return "all" if trips(15) >= 1 else "partial"


@dataclass(frozen=True)
class GN:
    G: int
    D: int
    xpat: str
    mspat: str

    @property
    def name(self):
        return f"graphnorm/g{self.G}d{self.D}/{self.xpat}.{self.mspat}"

    @property
    def grid_y(self):
        return -(-self.D // 256)


GN_CASES = tuple([GN(g, d, "normal", "rand") for g, d in GN_PAIRS] +
                 [GN(g, d, xp, mp) for g, d in GN_ALL_PATTERNS_AT for xp, mp in GN_PATTERNS[1:]])


def gn_sizes(c):
    """Group sizes from GN_SIZES: an empty group first, in the middle and last (G >= 4), one group of
    64 and one of 130 rows, the rest 0..3 rows."""
    g = _gen("sizes" + c.name)
    s = torch.tensor(GN_SIZES[:4])[torch.randint(0, 4, (c.G,), generator=g)]
    if c.G == 1:
        s[0] = 3
    elif c.G == 2:
        s[0], s[1] = 0, 64
    else:
        s[1], s[c.G // 3] = 64, 130
        if c.G >= 4:
            s[0] = s[c.G // 2] = s[c.G - 1] = 0
            s[2] = 2
    return s.tolist()


def gn_inputs(c):
    g = _gen(c.name)
    sizes = gn_sizes(c)
    off = [0]
    for n in sizes:
        off.append(off[-1] + n)
    N = off[-1]
    x = _randn(g, N, c.D)
    if c.xpat == "offset":
        x = x + 1000.0
    elif c.xpat == "const":
        for a, b in zip(off[:-1], off[1:]):
            if b > a:
                x[a:b] = x[a].clone() + 3.0
    ms = {"one": torch.ones(c.D), "zero": torch.zeros(c.D), "rand": 1.0 + 0.3 * _randn(g, c.D)}[c.mspat]
    w, b = 1.0 + 0.3 * _randn(g, c.D), _randn(g, c.D)
    if c.D >= 2:
        w[c.D // 2] = 0.0
    return {"off": off, "x": x, "w": w, "b": b, "ms": ms, "gy": _randn(g, N, c.D)}


def gn_eval(inp, dt=F64, absolute=False):
    """(y, g_x, g_w, g_b, g_ms) of norm.hip's formulas in dt; absolute: den of the same expressions
    (every term by its absolute value, the group's own var + eps kept as it is)."""
    x, w, b, ms, gy = (inp[k].to(dt) for k in ("x", "w", "b", "ms", "gy"))
    A = (lambda t: t.abs()) if absolute else (lambda t: t)
    D = x.shape[1]
    y, gx = torch.zeros_like(x), torch.zeros_like(x)
    gw, gb, gms = (torch.zeros(D, dtype=dt) for _ in range(3))
    eps = torch.tensor(EPS32, dtype=dt)
    for a, e in zip(inp["off"][:-1], inp["off"][1:]):
        n = e - a
        if n == 0:
            continue
        xs, gs = x[a:e], gy[a:e]
        mean_t = xs.sum(0) / n
        o_t = xs - mean_t * ms                                   # the true o: var is never "absolute"
        var = (o_t * o_t).sum(0) / n + eps
        inv = 1.0 / var.sqrt()
        mean = A(xs).sum(0) / n
        o = A(xs) + mean * A(ms) if absolute else o_t
        y[a:e] = A(w) * inv * o + A(b)
        sgy, sgyo, so = A(gs).sum(0), (A(gs) * o).sum(0), o.sum(0)
        k1, k2 = A(w) * inv, sgyo / (n * var)
        sum_go = k1 * (sgy + k2 * so) if absolute else k1 * (sgy - k2 * so)
        go = k1 * (A(gs) + k2 * o) if absolute else k1 * (gs - k2 * o)
        gx[a:e] = go + A(ms) * sum_go / n if absolute else go - ms * sum_go / n
        gw += sgyo * inv
        gb += sgy
        gms += mean * sum_go if absolute else -mean * sum_go
    return y, gx, gw, gb, gms


def gn_bars(c, inp, refs, dens):
    """Element-wise allowed |got - ref| for (y, g_x, g_w, g_b, g_ms)."""
    sizes = [e - a for a, e in zip(inp["off"][:-1], inp["off"][1:])]
    n_row = torch.tensor([n for n in sizes for _ in range(n)], dtype=F64)[:, None]
    nmax = max(sizes)
    out = []
    for i, (r, d) in enumerate(zip(refs, dens)):
        depth = (n_row + 8) if i < 2 else (nmax + c.G + 8)
        out.append(2.0 ** -23 * r.abs() + 2.0 * depth * 2.0 ** -53 * d)
    return out


# ====================================================================== LayerNorm
LN_D = (1, 3, 63, 64, 65, 127, 128, 129, 383, 384, 385, 448, 449, 511, 512)
LN_D_MORE = (192, 200, 256, 300, 320)      # three to five slots, the last one full and partly masked
LN_ROWS = (1, 3, 4, 5, 9)
LN_PATTERNS = ("normal", "offset", "const", "gzero")
# multiples of D (k = 0: D + 1) for (ldx, ldy, ldgy, ldgx): each pitch at D, D + 1 and 3 D
LN_PITCHES = ((1, 1, 1, 1), (0, 0, 0, 0), (3, 3, 3, 3), (1, 0, 3, 1), (3, 1, 0, 0), (0, 3, 1, 3))


@dataclass(frozen=True)
class LN:
    rows: int
    D: int
    pat: str
    pitch: tuple

    @property
    def name(self):
        return f"layernorm/r{self.rows}d{self.D}/{self.pat}/p{''.join(map(str, self.pitch))}"

    def ld(self, i):
        return self.D + 1 if self.pitch[i] == 0 else self.pitch[i] * self.D

    @property
    def slots(self):
        return -(-self.D // 64)


def _ln_cases():
    out, k = [], 0
    for i, D in enumerate(LN_D + LN_D_MORE):
        pats = LN_PATTERNS if D in (449, 512) else LN_PATTERNS[(2 * i) % 4:(2 * i) % 4 + 2]
        for pat in pats:
            out.append(LN(LN_ROWS[k % 5], D, pat, LN_PITCHES[k % 6]))
            k += 1
    out += [LN(r, 130, "normal", LN_PITCHES[r % 6]) for r in LN_ROWS]
    return tuple(out)


LN_CASES = _ln_cases()


def ln_inputs(c):
    g = _gen(c.name)
    x = _randn(g, c.rows, c.D)
    if c.pat == "offset":
        x = x + 1000.0
    elif c.pat == "const":
        x[0] = 2.5                       # var = 0: eps decides
        if c.rows > 2:
            x[2] = x[2, 0].clone()
    gamma, beta = 1.0 + 0.3 * _randn(g, c.D), _randn(g, c.D)
    if c.pat == "gzero":
        gamma[::2] = 0.0
    inp = {"x": x, "gamma": gamma, "beta": beta, "gy": _randn(g, c.rows, c.D)}
    _, mean, rstd = ln_fwd(inp)
    inp["mean"], inp["rstd"] = mean.float(), rstd.float()    # the backward's inputs, as fp32 values
    return inp


def ln_fwd(inp, dt=F64, absolute=False):
    """(y, mean, rstd); absolute: den (mean and rstd are their own den: |mean| <= sum |x| / D)."""
    x, gamma, beta = (inp[k].to(dt) for k in ("x", "gamma", "beta"))
    D = x.shape[1]
    mean = x.sum(1, keepdim=True) / D
    d = x - mean
    rstd = 1.0 / ((d * d).sum(1, keepdim=True) / D + torch.tensor(EPS32, dtype=dt)).sqrt()
    if absolute:
        ma = x.abs().sum(1, keepdim=True) / D
        return (x.abs() + ma) * rstd * gamma.abs() + beta.abs(), ma[:, 0], rstd[:, 0]
    return d * rstd * gamma + beta, mean[:, 0], rstd[:, 0]


def ln_bwd(inp, dt=F64, absolute=False, mean=None, rstd=None):
    """(g_x, g_y_xhat) from the given mean / rstd (default: the fp32 values the kernel is given)."""
    x, gamma, gy = (inp[k].to(dt) for k in ("x", "gamma", "gy"))
    mean = (inp["mean"] if mean is None else mean).to(dt)[:, None]
    rstd = (inp["rstd"] if rstd is None else rstd).to(dt)[:, None]
    D = x.shape[1]
    if absolute:
        xh, g = (x.abs() + mean.abs()) * rstd, gy.abs() * gamma.abs()
        m1, m2 = g.sum(1, keepdim=True) / D, (g * xh).sum(1, keepdim=True) / D
        return rstd * (g + m1 + xh * m2), gy.abs() * xh
    xh, g = (x - mean) * rstd, gy * gamma
    m1, m2 = g.sum(1, keepdim=True) / D, (g * xh).sum(1, keepdim=True) / D
    return rstd * (g - m1 - xh * m2), gy * xh


# ====================================================================== plain token attention
AT_DK = (16, 20, 64, 68, 128, 132, 192, 196, 256, 260, 320, 324, 380, 384)
AT_HB = ((1, 1), (3, 1), (12, 1), (1, 2), (3, 2), (1, 5), (3, 5), (12, 2))   # B H % 4: 1 3 0 2 2 1 3 0
AT_PATTERNS = ("normal", "equal", "saturated")


def by_width(dk):
    """fusion_common.h by_width: the kernel instance (kMask, kV)."""
    return (False, 6) if dk == 384 else (True, -(-dk // 64))


@dataclass(frozen=True)
class AT:
    B: int
    H: int
    dk: int
    pat: str
    pad: int                  # ld = 3 H dk + pad
    padg: int

    @property
    def name(self):
        return f"token_attn/b{self.B}h{self.H}dk{self.dk}/{self.pat}/p{self.pad}.{self.padg}"

    @property
    def W(self):
        return 3 * self.H * self.dk


def _at_cases():
    out, k = [], 0
    for dk in AT_DK:
        for pat in AT_PATTERNS:
            H, B = AT_HB[k % len(AT_HB)]
            out.append(AT(B, H, dk, pat, 4 * (k % 2), 4 * ((k // 2) % 2)))
            k += 1
    return tuple(out)


AT_CASES = _at_cases()


def at_inputs(c):
    """qkv [3 B, 3 H dk], g_att [B, H, 3, dk]; P32 [B, H, 3, 3]: the backward's fp32 input."""
    g = _gen(c.name)
    qkv = _randn(g, c.B, 3, 3, c.H, c.dk)                 # (b, token, q|k|v, h, dk)
    if c.pat == "equal":                                  # one q and one k per (b, h): nine equal scores
        qkv[:, :, 0] = qkv[:, :1, 0].clone()
        qkv[:, :, 1] = qkv[:, :1, 1].clone()
    elif c.pat == "saturated":                            # k_t = a_t q_0-ish: row scores 130 apart
        q0 = torch.sign(_randn(g, c.B, 1, c.H, c.dk))
        qkv[:, :, 0] = q0 * (1.0 + 0.01 * _randn(g, c.B, 3, c.H, c.dk))
        lead = torch.tensor([130.0, 0.0, -130.0])[None, :, None, None] / math.sqrt(c.dk)
        qkv[:, :, 1] = q0 * lead + 0.01 * _randn(g, c.B, 3, c.H, c.dk)
    inp = {"qkv": qkv.reshape(3 * c.B, c.W), "g_att": _randn(g, c.B, c.H, 3, c.dk),
           "scale": float(torch.tensor(1.0 / math.sqrt(c.dk), dtype=F32))}
    inp["P32"] = at_fwd(c, inp)[1].float()
    return inp


def _qkv(c, inp, dt):
    t = inp["qkv"].to(dt).reshape(c.B, 3, 3, c.H, c.dk).permute(2, 0, 3, 1, 4)   # (3, B, H, token, dk)
    return t[0], t[1], t[2]


def at_fwd(c, inp, dt=F64, absolute=False):
    """(att [B, H, 3, dk], P [B, H, 3, 3]); absolute: their den (see the module docstring)."""
    q, k, v = _qkv(c, inp, dt)
    s = (q @ k.transpose(-1, -2)) * inp["scale"]
    P = torch.softmax(s, -1)
    if not absolute:
        return P @ v, P
    sA = (q.abs() @ k.abs().transpose(-1, -2)) * inp["scale"]
    dP = P * (1.0 + sA + (P * sA).sum(-1, keepdim=True))
    return dP @ v.abs(), dP


def at_bwd(c, inp, dt=F64, absolute=False, P=None):
    """g_qkv [3 B, 3 H dk] from the given P (default: the fp32 P the kernel is given)."""
    q, k, v = _qkv(c, inp, dt)
    P = (inp["P32"] if P is None else P).to(dt)
    g = inp["g_att"].to(dt)
    sc = inp["scale"]
    if absolute:
        q, k, v, g = q.abs(), k.abs(), v.abs(), g.abs()
    gp = g @ v.transpose(-1, -2)                          # [.., a, c]
    dot = (P * gp).sum(-1, keepdim=True)
    gs = P * (gp + dot if absolute else gp - dot) * sc
    gv = P.transpose(-1, -2) @ g
    gq = gs @ k
    gk = gs.transpose(-1, -2) @ q
    out = torch.stack([gq, gk, gv])                       # (3, B, H, token, dk)
    return out.permute(1, 3, 0, 2, 4).reshape(3 * c.B, c.W)


# ====================================================================== BCE with logits
BCE_N = (1, 255, 256, 257, 1000)
BCE_PLANTED = (0.0, 1e-8, -1e-8, 20.0, -20.0, 88.0, -88.0, 89.0, -89.0, 104.0, -104.0, 1e4, -1e4)


@dataclass(frozen=True)
class BCE:
    n: int
    soft: bool

    @property
    def name(self):
        return f"bce/{self.n}/{'soft' if self.soft else 'hard'}"


BCE_CASES = tuple(BCE(n, s) for s in (False, True) for n in BCE_N)


def bce_inputs(c):
    g = _gen(c.name)
    z = 3.0 * _randn(g, c.n)
    if c.n == 1:
        z[0] = 89.0 if c.soft else -89.0
    else:                                                 # every planted value with y = 0 / 1 (or two soft labels)
        pl = torch.tensor(BCE_PLANTED, dtype=F32).repeat(2)
        z[3:3 + pl.numel()] = pl
    y = torch.rand(c.n, generator=g) if c.soft else (torch.rand(c.n, generator=g) < 0.5).float()
    if c.n > 1:
        y[3:3 + len(BCE_PLANTED)] = 0.25 if c.soft else 0.0
        y[3 + len(BCE_PLANTED):3 + 2 * len(BCE_PLANTED)] = 1.0
    return {"z": z, "y": y}


def bce_eval(inp, dt=F64, absolute=False):
    """(loss_terms, g_z) in the kernel's form."""
    z, y = inp["z"].to(dt), inp["y"].to(dt)
    n = z.numel()
    l1p = torch.log1p(torch.exp(-z.abs()))
    sig = 1.0 / (1.0 + torch.exp(-z))
    if absolute:
        return z.clamp_min(0) + z.abs() * y.abs() + l1p, (sig + y.abs()) / n
    return z.clamp_min(0) - z * y + l1p, (sig - y) / n


# ====================================================================== relu_bwd, add_cols
RELU_N = (1, 255, 256, 257, 16384 * 256 + 3)              # the last: the grid cap's second sweep
RELU_GRID_CAP = 16384 * 256
RELU_SCALES = (1.0, 2.0, float(torch.tensor(1.0 / 0.7, dtype=F32)))
DENORMAL = 2.0 ** -140


def relu_inputs(n):
    g = _gen(f"relu{n}")
    y, gy = _randn(g, n), _randn(g, n)
    sp = torch.tensor([0.0, -0.0, -1.5, DENORMAL, float("nan"), 1.0], dtype=F32)
    for base in (0, 252, n - 6):                          # at the start, across a block edge, in the last sweep
        if 0 <= base and base + 6 <= n:
            y[base:base + 6] = sp
    if n == 1:
        y[0] = DENORMAL
    return {"y": y, "gy": gy}


def relu_expected(inp, scale):
    """The fp32 CPU expression: one IEEE multiply (none at scale 1), +0 where y is not > 0."""
    gy = inp["gy"]
    passed = gy if scale == 1.0 else gy * torch.tensor(scale, dtype=F32)
    return torch.where(inp["y"] > 0, passed, torch.zeros_like(gy))


ADD_COLS_CASES = tuple((r, c, c + ps, c + pd) for r in (1, 5) for c in (4, 260) for ps in (0, 4) for pd in (0, 4))


# ====================================================================== optimizer pair
OPT_SIZES = (0, 1, 3, 4, 5, 16383, 16384, 16385, 40000)
OPT_CHUNKS = (16384, 100)
OPT_STEPS = (0, 1, 9, 999, 100000)
OPT_FLAGS = (1.0, 0.0, 2.0, 1.0, 1.0)
OPT_HYPER = tuple((wd, gs, betas) for wd in (0.0, 1e-4)
                  for gs in (1.0, 0.5, float(torch.tensor(1.0 / 3.0, dtype=F32)))
                  for betas in ((0.9, 0.999), (0.0, 0.0)))


def _sizes_300():
    s = [OPT_SIZES[i % 5] for i in range(300)]
    s[7], s[150], s[260], s[299] = 16383, 16385, 16384, 40000        # (150: flag 0, skipped in both its chunks)
    return tuple(s)


OPT_LAYOUTS = {"p1": (40000,), "p3a": (16383, 16384, 16385), "p3b": (0, 5, 40000), "p300": _sizes_300()}


@dataclass(frozen=True)
class OPT:
    layout: str
    chunk: int
    wd: float
    gs: float
    betas: tuple
    lr: float = 1e-3
    eps: float = 1e-8

    @property
    def name(self):
        return f"adam/{self.layout}/c{self.chunk}/wd{self.wd}gs{self.gs:.3f}b{self.betas[0]}"

    @property
    def sizes(self):
        return OPT_LAYOUTS[self.layout]

    @property
    def P(self):
        return len(self.sizes)


def _opt_cases():
    lay = [(n, ch) for n in OPT_LAYOUTS for ch in OPT_CHUNKS]
    return tuple(OPT(n, ch, *OPT_HYPER[j]) for i, (n, ch) in enumerate(lay) for j in range(len(OPT_HYPER))
                 if (i + j) % 4 == 0)


OPT_CASES = _opt_cases()


def opt_tables(sizes, chunk):
    """A hand-built table: segments start 16-B aligned with 0..3 pad floats between them (and a
    whole extra pad quad after every third), `chunk` elements per chunk, one empty chunk for an
    empty parameter.  (chunk_param, chunk_beg, chunk_end, param_off, numel)."""
    off, o = [], 0
    for i, n in enumerate(sizes):
        off.append(o)
        o += (n + 3) // 4 * 4 + (4 if i % 3 == 2 else 0)
    cp, cb, ce = [], [], []
    for i, (o_, n) in enumerate(zip(off, sizes)):
        for b in range(o_, o_ + max(n, 1), chunk):
            cp.append(i)
            cb.append(b)
            ce.append(min(o_ + n, b + chunk))
    return cp, cb, ce, off, o


def tables_ok(sizes, cp, cb, ce, off, numel=None):
    """The contract: chunks tile each segment exactly, never straddle, offsets % 4 == 0, segments
    disjoint and in range."""
    cover = {i: [] for i in range(len(sizes))}
    for i, b, e in zip(cp, cb, ce):
        if not (0 <= i < len(sizes) and off[i] <= b <= e <= off[i] + sizes[i]):
            return False
        cover[i].append((b, e))
    for i, n in enumerate(sizes):
        if off[i] % 4 or (numel is not None and off[i] + n > numel):
            return False
        if i and off[i] < off[i - 1] + sizes[i - 1]:
            return False
        pos = off[i]
        for b, e in sorted(cover[i]):
            if b != pos:
                return False
            pos = e
        if pos != off[i] + n:
            return False
    return True


def opt_inputs(c):
    """Per parameter: p, g, m, v (fp32), flag, preset step.  Step 0 goes with zero moments."""
    g = _gen(c.name)
    ps = []
    for i, n in enumerate(c.sizes):
        step = OPT_STEPS[(i + i // 5) % 5]
        m = 0.1 * _randn(g, n) if step else torch.zeros(n)
        v = 0.01 * torch.rand(n, generator=g) if step else torch.zeros(n)
        ps.append({"p": _randn(g, n), "g": _randn(g, n), "m": m, "v": v, "flag": OPT_FLAGS[(i + i // 5 // 5) % 5],
                   "step": step})
    return ps


def adam_eval(c, q, dt=F64, absolute=False):
    """(p, m, v) after one step of parameter record q, in adam_flat_kernel's form.  In float32 the
    scalars are formed as the kernel forms them (in double, rounded once)."""
    b1, b2 = c.betas
    step = q["step"] + 1
    bc1, bc2 = 1.0 - b1 ** step, 1.0 - b2 ** step
    f = (lambda s: float(torch.tensor(s, dtype=F32))) if dt == F32 else (lambda s: s)
    step_size, bc2s, w1, w2, b2f = f(c.lr / bc1), f(math.sqrt(bc2)), f(1.0 - b1), f(1.0 - b2), f(b2)
    wd, eps, gs = f(c.wd), f(c.eps), c.gs
    p, g, m, v = (q[k].to(dt) for k in ("p", "g", "m", "v"))
    if absolute:
        p, g, m = p.abs(), g.abs(), m.abs()
    g = g * gs + wd * p
    v1 = v * b2f + w2 * g * g
    if absolute:
        m1 = m + w1 * (g + m)
        denom = adam_eval(c, q, dt)[2].sqrt() / bc2s + eps        # the true denominator
        return p + step_size * (m1 / denom), m1, v1
    m1 = m + w1 * (g - m)
    denom = v1.sqrt() / bc2s + eps
    return p - step_size * (m1 / denom), m1, v1


# ====================================================================== the refusals
INVALID, WORKSPACE = 1, 3


def refusals(P1, P1_off):
    """{id: (entry, the word mvml_last_error() must hold, code, args)} of every documented refusal of the
    entries; P1 stands for every pointer (16-byte aligned, P1_off 4 bytes past it), `None` is the NULL
    under test, the last argument the stream."""
    out = {}

    def add(entry, who, names, good, **extra):
        for i, n in enumerate(names):
            if n:
                out[f"{entry}:{n} NULL"] = (entry, who, INVALID, [None if j == i else a for j, a in enumerate(good)])
        for k, (i, v) in extra.items():
            out[f"{entry}:{k}"] = (entry, who, INVALID, [v if j == i else a for j, a in enumerate(good)])

    f = 1e-5
    add("mvml_graphnorm_fwd", "graphnorm_fwd", ("", "", "group_offsets", "x", "weight", "bias", "mean_scale", "", "y", ""),
        [2, 8, P1, P1, P1, P1, P1, f, P1, None], **{"D=0": (1, 0), "G<0": (0, -1)})
    add("mvml_graphnorm_bwd", "graphnorm_bwd",
        ("", "", "group_offsets", "x", "weight", "mean_scale", "", "g_y", "g_x", "", "", "", "", "", ""),
        [2, 8, P1, P1, P1, P1, f, P1, P1, P1, P1, P1, P1, 1 << 20, None], **{"D=0": (1, 0)})
    out["mvml_graphnorm_bwd:workspace NULL"] = ("mvml_graphnorm_bwd", "graphnorm_bwd", WORKSPACE,
                                                [2, 8, P1, P1, P1, P1, f, P1, P1, P1, P1, P1, None, 1 << 20, None])
    out["mvml_graphnorm_bwd:workspace short"] = ("mvml_graphnorm_bwd", "graphnorm_bwd", WORKSPACE,
                                                 [2, 8, P1, P1, P1, P1, f, P1, P1, P1, P1, P1, P1, 3 * 2 * 8 * 8 - 1, None])
    add("mvml_layernorm_fwd", "layernorm_fwd", ("", "", "x", "", "gamma", "beta", "", "y", "", "mean", "rstd", ""),
        [3, 8, P1, 8, P1, P1, f, P1, 8, P1, P1, None], **{"D=0": (1, 0), "D=513": (1, 513), "ldx<D": (3, 7), "ldy<D": (8, 7)})
    add("mvml_layernorm_bwd", "layernorm_bwd",
        ("", "", "x", "", "gamma", "mean", "rstd", "g_y", "", "g_x", "", "g_y_xhat", ""),
        [3, 8, P1, 8, P1, P1, P1, P1, 8, P1, 8, P1, None],
        **{"D=0": (1, 0), "D=513": (1, 513), "ldx<D": (3, 7), "ldgy<D": (8, 7), "ldgx<D": (10, 7)})
    add("mvml_token_attn_fwd", "token_attn_fwd", ("", "", "", "qkv", "", "", "att", "P", ""),
        [2, 2, 16, P1, 96, 0.25, P1, P1, None], **{"dk=18": (2, 18), "dk=388": (2, 388), "H=0": (1, 0), "ld<3Hdk": (4, 95)})
    add("mvml_token_attn_bwd", "token_attn_bwd", ("", "", "", "qkv", "", "", "P", "g_att", "g_qkv", "", ""),
        [2, 2, 16, P1, 96, 0.25, P1, P1, P1, 96, None],
        **{"dk=18": (2, 18), "H=0": (1, 0), "ld<3Hdk": (4, 95), "ldg<3Hdk": (9, 95)})
    add("mvml_bce_logits", "bce_logits", ("", "z", "y", "loss_terms", "g_z", ""), [5, P1, P1, P1, P1, None], **{"n<0": (0, -1)})
    add("mvml_relu_bwd", "relu_bwd", ("", "y", "g_y", "g_x", "", ""), [5, P1, P1, P1, 1.0, None], **{"n<0": (0, -1)})
    add("mvml_add_cols_f32", "add_cols", ("", "", "src", "", "dst", "", ""), [2, 8, P1, 8, P1, 8, None],
        **{"cols=0": (1, 0), "cols%4": (1, 6), "lds<cols": (3, 4), "ldd<cols": (5, 4), "lds%4": (3, 9),
           "src misaligned": (2, P1_off), "dst misaligned": (4, P1_off)})
    add("mvml_grad_gather", "grad_gather",
        ("", "chunk_param", "chunk_beg", "chunk_end", "param_off", "src", "", "flat", "", ""),
        [1, P1, P1, P1, P1, P1, 1, P1, 8, None], **{"nchunks<0": (0, -1), "P<0": (6, -1), "numel<0": (8, -1)})
    add("mvml_adam_flat", "adam_flat",
        ("", "chunk_param", "chunk_beg", "chunk_end", "flags", "steps", "", "param", "grad", "exp_avg", "exp_avg_sq",
         "", "", "", "", "", "", ""),
        [1, P1, P1, P1, P1, P1, 1, P1, P1, P1, P1, 1e-3, 0.9, 0.999, 1e-8, 0.0, 1.0, None],
        **{"nchunks<0": (0, -1), "beta1=1": (12, 1.0), "beta2<0": (13, -0.1), "eps<0": (14, -1.0), "lr<0": (11, -1.0)})
    return out
