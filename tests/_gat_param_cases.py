"""Case tables, input makers, float64 references and bars for the parameter side of a GAT layer at
the ABI (csrc/gat_params.hip and the projection's logit-partial epilogue in csrc/gemm_f32.hip).
No GPU import: the CPU conditions are in test_gat_param_cases_cpu.py, the GPU comparisons in
test_gpu_gat_params.py.  The method is _gemm_cases.py's: kind (a) inputs are exact (small integers,
A-side rows times 2^-e), so the float64 result cast to fp32 is the only right answer on any path;
kind (b) inputs are randn and held element-wise to a bar derived per kernel:

  mvml_gat_proj_fwd   Y: bar(e_cpu) of _gemm_cases; elr: bar(e_cpu_el), den_el = sum_f (|X||W|^T) |a|
  fold_weights        MEAN rows H 2^-24 den (H - 1 adds, one divide); A rows F 2^-24 den (F fmas)
  unfold_grads        g_fc 2 * 2^-24 den (two fmas); g_res bitwise, or 2^-24 |ref| (MEAN, H = 3)
  attn_grad           depth 2^-24 den, depth = ceil(rows_per / 4) + 2 + S (attn_grad_plan)
  head_mean           H 2^-24 den; backward bitwise, or 2^-24 |ref| at H = 3
"""
import zlib
from dataclasses import dataclass

import torch

from _gemm_cases import amax_shift, split2h  # noqa: F401  (the CPU conditions use them)

U = 2.0 ** -24                # unit roundoff of fp32
RES_PROJ, RES_MEAN, RES_NONE = 0, 1, 2
ALGO = {"f32": 0, "x3": 1, "bf16": 2, "f16x2": 3}   # MVML_GEMM_*


def proj_logw(F):
    """common.h proj_logw: log2 of the largest power of two <= 32 dividing F."""
    lw = 0
    while lw < 5 and F % (2 << lw) == 0:
        lw += 1
    return lw


def proj_cols(H, F, res):
    return H * F + (0 if res == RES_NONE else F if res == RES_MEAN else H * F)


def _gen(name, kind):
    return torch.Generator().manual_seed(zlib.crc32((name + kind).encode()))


def _ints(g, shape, lim=8):
    return torch.randint(-lim, lim + 1, shape, generator=g).float()


# ====================================================================== 1. mvml_gat_proj_fwd
@dataclass(frozen=True)
class Proj:
    algo: str                 # f32 | x3 | bf16 | f16x2
    tile: int                 # forced gemm_tile: 128 | 256
    N: int
    K: int
    H: int
    F: int
    res: int
    pad_x: int = 0            # ldx = K + pad_x
    pad_w: int = 0
    off_x: int = 0            # X's base in floats past a 16-B aligned address
    persist: int = -1         # gemm_persist, -1: the default
    maxima: str = "given"     # f16x2 at tile 256: given | null | one

    @property
    def name(self):
        return (f"proj/{self.algo}/t{self.tile}/{self.N}x{self.K}/h{self.H}f{self.F}r{self.res}/"
                f"p{self.pad_x}.{self.pad_w}o{self.off_x}/ps{self.persist}/{self.maxima}")

    @property
    def ldx(self):
        return self.K + self.pad_x

    @property
    def ldw(self):
        return self.K + self.pad_w

    @property
    def HF(self):
        return self.H * self.F

    @property
    def C(self):
        return proj_cols(self.H, self.F, self.res)

    @property
    def wide(self):
        """gemm_proj_epi: bf16 exists only in the 256x256 kernel; x3 / f16x2 follow the forced tile."""
        return self.algo == "bf16" or (self.algo in ("x3", "f16x2") and self.tile == 256)

    @property
    def fast(self):
        """x3w_fast of two K-contiguous operands (Wcat's base is 16-B aligned)."""
        return self.ldx % 4 == 0 and self.off_x % 4 == 0 and self.ldw % 4 == 0 and self.K % 4 == 0

    @property
    def labels(self):
        """The kernel instance gemm_proj_epi launches: (algo, forced tile, alignment and K % 4,
        proj_logw(F)) alone decide it."""
        lw = proj_logw(self.F)
        if self.algo == "f32":
            return (f"f32-lw{lw}",)
        if not self.wide:       # split-fp16 exists only in the 256x256 kernel: f16x2 runs split-bf16
            return (f"x3s-lw{lw}",) + ((f"x3s-from-f16x2-lw{lw}",) if self.algo == "f16x2" else ())
        return (f"x3w-{self.algo}-{'fast' if self.fast else 'guarded'}-lw{lw}",)

    @property
    def emax(self):
        return 8 if self.algo == "f16x2" else 20   # f16x2: ONE power of two scales all of X

    @property
    def attn_lim(self):
        return 8 if self.K * self.F <= 7600 else 4

    def kinds(self):
        return "a" if self.algo == "bf16" else "ab"


PROJ_REQUIRED_LABELS = tuple(
    [f"f32-lw{lw}" for lw in (2, 3, 4, 5)] + [f"x3s-lw{lw}" for lw in (2, 3, 4, 5)] +
    [f"x3s-from-f16x2-lw{lw}" for lw in (2, 3, 4, 5)] +
    [f"x3w-{a}-{p}-lw{lw}" for a in ("bf16", "f16x2", "x3") for p in ("fast", "guarded") for lw in (2, 3, 4, 5)])
PROJ_INSTANCES = tuple(lab for lab in PROJ_REQUIRED_LABELS if "from" not in lab)   # the 32

# (algo, forced tile): the six ways into gemm_proj_epi
PROJ_PATHS = (("f32", 128), ("x3", 128), ("f16x2", 128), ("bf16", 256), ("f16x2", 256), ("x3", 256))
# F = 4 / 24 / 48 / 96: W = 4 / 8 / 16 / 32; every H and every residual layout rides along
PROJ_WIDTHS = ((1, 4, RES_MEAN), (2, 24, RES_PROJ), (4, 48, RES_NONE), (8, 96, RES_MEAN))
PROJ_ROWS = (1, 31, 33, 127, 129, 255, 257)


def _proj_cases():
    out = []
    for algo, tile in PROJ_PATHS:
        def P(N, K, hfr, **kw):
            out.append(Proj(algo, tile, N, K, *hfr, **kw))
        for hfr in PROJ_WIDTHS:
            P(257, 76, hfr)                          # K = 76, ldx = ldw = 76: fast
            P(257, 74, hfr, pad_x=2, pad_w=2)        # aligned pitch 76 but K % 4 != 0: guarded
        for n in PROJ_ROWS:
            P(n, 76, (2, 24, RES_MEAN))
        w8 = (2, 24, RES_MEAN)
        P(129, 75, w8)                               # pitch 75: guarded
        P(129, 76, w8, off_x=1)                      # a base one float off 16 B: guarded
        P(129, 4, (8, 4, RES_PROJ))                  # K shorter than one k-tile
        P(129, 16, (1, 48, RES_PROJ))                # K equal to one k-tile (x3w) / half of one
        P(129, 80, (4, 96, RES_NONE), pad_x=4, pad_w=4)
        # H*F ends inside a 32-column block, a 128 tile and a 256 tile: gc < cols and cb0 >= cols decide
        P(33, 76, (1, 4, RES_MEAN))                  # H*F = 4, C = 8
        P(33, 76, (1, 24, RES_PROJ))                 # H*F = 24, C = 48
        P(33, 76, (1, 24, RES_NONE))                 # H*F = C = 24
        P(33, 76, (2, 24, RES_NONE))                 # H*F = C = 48
        P(33, 76, (1, 48, RES_MEAN))                 # H*F = 48, C = 96
        P(130, 76, (4, 96, RES_PROJ))                # H*F = 384, C = 768
        if tile == 256 or algo == "bf16":
            # 3 x 6 = 18 tiles: more than the persistent cap of 8; and one workgroup per tile
            P(520, 76, (8, 96, RES_PROJ), persist=8)
            P(520, 74, (8, 96, RES_PROJ), pad_x=2, pad_w=2, persist=8)
            P(520, 76, (8, 96, RES_PROJ), persist=0)
    return out


PROJ_CASES = _proj_cases()
# the maxima of MVML_GEMM_F16X2 at tile 256: supplied, computed here, or only one supplied
PROJ_MAXIMA = tuple(Proj("f16x2", 256, 200, k, 2, 24, RES_MEAN, pad_x=p, pad_w=p, maxima=m)
                    for k, p in ((76, 0), (74, 2)) for m in ("given", "null", "one"))


def proj_groups():
    out = {}
    for c in PROJ_CASES:
        out.setdefault(f"{c.algo}-t{c.tile}", []).append(c)
    return out


def proj_inputs(c, kind):
    """X [N, K] (rows times 2^-e; one all-zero row), Wcat [C, K], attn [2, H*F], e [N]."""
    g = _gen(c.name, kind)
    e = torch.randint(0, c.emax + 1, (c.N, 1), generator=g)
    if c.N >= 2:
        e[0], e[c.N - 1] = 0, c.emax
    scale = torch.pow(2.0, -e.float())
    if kind == "a":
        X = _ints(g, (c.N, c.K)) * scale
        W = _ints(g, (c.C, c.K))
        a = _ints(g, (2, c.HF), c.attn_lim)
    else:
        X = torch.randn((c.N, c.K), generator=g) * scale
        W = torch.randn((c.C, c.K), generator=g) / c.K ** 0.5
        a = torch.randn((2, c.HF), generator=g)
    if c.N >= 3:
        X[c.N // 2] = 0.0
    return {"X": X, "W": W, "a": a, "e": e.reshape(-1)}


def _proj_eval(c, X, W, a):
    Y = X @ W.t()
    Z = Y[:, :c.HF].reshape(c.N, c.H, c.F)
    av = a.reshape(2, 1, c.H, c.F)
    return Y, torch.cat([(Z * av[0]).sum(-1), (Z * av[1]).sum(-1)], 1)


def proj_reference(c, inp):
    """float64 (Y [N, C], elr [N, 2H], den_y, den_el)."""
    X, W, a = (inp[k].double() for k in ("X", "W", "a"))
    Y, elr = _proj_eval(c, X, W, a)
    den_y, den_el = _proj_eval(c, X.abs(), W.abs(), a.abs())
    return Y, elr, den_y, den_el


def proj_cpu_fp32(c, inp):
    """torch's CPU fp32 evaluation of the same two expressions."""
    return _proj_eval(c, inp["X"], inp["W"], inp["a"])


def proj_epilogue_emulation(c, Y32, a):
    """elr from an fp32 Y in the epilogue's own order: per W-column group the halving butterfly
    (pairs at distance W/2, W/4, .. 1), then a head's F / W partials in sequence."""
    W = 1 << proj_logw(c.F)
    out = []
    for side in (0, 1):
        v = (Y32[:, :c.HF] * a[side]).reshape(c.N, c.HF // W, W)
        w = W
        while w > 1:
            w //= 2
            v = v[:, :, :w] + v[:, :, w:2 * w]
        part = v.reshape(c.N, c.H, c.F // W)
        acc = part[:, :, 0].clone()
        for b in range(1, c.F // W):
            acc = acc + part[:, :, b]
        out.append(acc)
    return torch.cat(out, 1)


# ====================================================================== 2 / 3. fold and unfold
@dataclass(frozen=True)
class Fold:
    H: int
    F: int
    Fin: int
    pad: int                  # ldw = Fin + pad
    res: int
    attn: bool

    @property
    def name(self):
        return f"fold/h{self.H}f{self.F}/k{self.Fin}+{self.pad}/r{self.res}a{int(self.attn)}"

    @property
    def ld(self):
        return self.Fin + self.pad

    @property
    def HF(self):
        return self.H * self.F

    @property
    def C(self):
        return proj_cols(self.H, self.F, self.res)

    @property
    def rows(self):
        return self.C + (2 * self.H if self.attn else 0)


FOLD_HF = ((1, 4), (2, 24), (4, 48), (8, 96), (3, 4))
FOLD_FIN = (1, 74, 75, 76)
FOLD_GRID_CAP = 8192 * 256    # the helper kernels' grid: more elements make a second pass


def _fold_cases():
    out = []
    for H, F in FOLD_HF:
        for Fin in FOLD_FIN:
            for pad in ((-Fin) % 4, 8):
                for res in (RES_PROJ, RES_MEAN, RES_NONE):
                    for attn in (True, False) if pad != 8 else (True,):
                        out.append(Fold(H, F, Fin, pad, res, attn))
    out.append(Fold(8, 96, 1400, 0, RES_PROJ, True))   # the grid-stride loop's second pass
    return out


FOLD_CASES = _fold_cases()


def fold_inputs(c, kind):
    """fc [HF, Fin], res [HF, Fin] (kind a: integer multiples of H, so the head mean is exact at
    H = 3 too), attn [2, HF]."""
    g = _gen(c.name, kind)
    if kind == "a":
        return {"fc": _ints(g, (c.HF, c.Fin)), "res": _ints(g, (c.HF, c.Fin)) * c.H, "a": _ints(g, (2, c.HF))}
    return {"fc": torch.randn((c.HF, c.Fin), generator=g), "res": torch.randn((c.HF, c.Fin), generator=g),
            "a": torch.randn((2, c.HF), generator=g)}


def fold_reference(c, fc, res, a):
    """float64 Wcat [rows, Fin] of the logical columns, and den of the same expression."""
    def ev(fc, res, a, mean_div):
        parts = [fc]
        if c.res == RES_PROJ:
            parts.append(res)
        elif c.res == RES_MEAN:
            parts.append(res.reshape(c.H, c.F, c.Fin).sum(0) / mean_div)
        if c.attn:
            w = fc.reshape(1, c.H, c.F, c.Fin)
            parts.append((a.reshape(2, c.H, c.F, 1) * w).sum(2).reshape(2 * c.H, c.Fin))
        return torch.cat(parts, 0)
    fc, res, a = fc.double(), res.double(), a.double()
    return ev(fc, res, a, c.H), ev(fc.abs(), res.abs(), a.abs(), c.H)


def fold_bar(c):
    """[rows] factor of den: 0 for the copied rows (bitwise), H u for MEAN rows, F u for A rows."""
    b = torch.zeros(c.rows, dtype=torch.float64)
    if c.res == RES_MEAN:
        b[c.HF:c.C] = c.H * U
    if c.attn:
        b[c.C:] = c.F * U
    return b


def _fma32(a, b, acc):
    return (a.double() * b.double() + acc.double()).float()


def fold_emulation(c, fc, res, a):
    """fold_weights_kernel in fp32, in its order: heads summed in sequence then / H; F fmas."""
    parts = [fc]
    if c.res == RES_PROJ:
        parts.append(res)
    elif c.res == RES_MEAN:
        r = res.reshape(c.H, c.F, c.Fin)
        s = torch.zeros((c.F, c.Fin))
        for h in range(c.H):
            s = s + r[h]
        parts.append(s / float(c.H))
    if c.attn:
        w = fc.reshape(c.H, c.F, c.Fin)
        av = a.reshape(2, c.H, c.F, 1)
        for side in (0, 1):
            acc = torch.zeros((c.H, c.Fin))
            for f in range(c.F):
                acc = _fma32(av[side, :, f], w[:, f], acc)
            parts.append(acc)
    return torch.cat(parts, 0)


def unfold_inputs(c, kind):
    """gW [rows, Fin] (kind a: the MEAN rows integer multiples of H), attn [2, HF]."""
    g = _gen("un" + c.name, kind)
    if kind == "a":
        gW = _ints(g, (c.rows, c.Fin))
        if c.res == RES_MEAN:
            gW[c.HF:c.C] *= c.H
        return {"gW": gW, "a": _ints(g, (2, c.HF))}
    return {"gW": torch.randn((c.rows, c.Fin), generator=g), "a": torch.randn((2, c.HF), generator=g)}


def unfold_reference(c, gW, a):
    """float64 (g_fc [HF, Fin], g_res [HF, Fin] | None, den of g_fc)."""
    gW, a = gW.double(), a.double()
    g_fc, den = gW[:c.HF].clone(), gW[:c.HF].abs()
    if c.attn:
        h = torch.arange(c.HF) // c.F
        gl, gr = gW[c.C + h], gW[c.C + c.H + h]
        g_fc = g_fc + a[0][:, None] * gl + a[1][:, None] * gr
        den = den + a[0].abs()[:, None] * gl.abs() + a[1].abs()[:, None] * gr.abs()
    if c.res == RES_PROJ:
        g_res = gW[c.HF:2 * c.HF].clone()
    elif c.res == RES_MEAN:
        g_res = (gW[c.HF:c.HF + c.F] / c.H).repeat(c.H, 1)
    else:
        g_res = None
    return g_fc, g_res, den


def unfold_emulation(c, gW, a):
    """unfold_w_kernel's g_fc in fp32: two fmas onto gW[r]."""
    gf = gW[:c.HF].clone()
    if c.attn:
        h = torch.arange(c.HF) // c.F
        gf = _fma32(a[0][:, None], gW[c.C + h], gf)
        gf = _fma32(a[1][:, None], gW[c.C + c.H + h], gf)
    return gf


def pow2(n):
    return n & (n - 1) == 0


# ====================================================================== 4. mvml_gat_attn_grad
def attn_grad_plan(N, HF):
    """gat_params.hip attn_grad_splits and the bar's depth: (S, rows_per, depth)."""
    cb = -(-HF // 256)
    S = max(1, min(-(-2048 // cb), -(-N // 256)))
    rows_per = -(-max(N, 1) // S)
    return S, rows_per, -(-rows_per // 4) + 2 + S


@dataclass(frozen=True)
class AttnGrad:
    N: int
    H: int
    F: int
    depth: int                # stated here, checked against attn_grad_plan on the CPU
    pad_y: int = 4            # ldy = H F + pad_y
    pad_g: int = 3            # ldgl = 2 H + pad_g

    @property
    def name(self):
        return f"attn_grad/{self.N}/h{self.H}f{self.F}/p{self.pad_y}.{self.pad_g}"

    @property
    def HF(self):
        return self.H * self.F


ATTN_GRAD_CASES = (
    # rows: every boundary of the split plan and the 4-row unroll, at two column blocks (4 live lanes)
    AttnGrad(0, 2, 130, 4), AttnGrad(1, 2, 130, 4), AttnGrad(3, 2, 130, 4), AttnGrad(4, 2, 130, 4),
    AttnGrad(5, 2, 130, 5), AttnGrad(255, 2, 130, 67), AttnGrad(256, 2, 130, 67), AttnGrad(257, 2, 130, 37),
    AttnGrad(1025, 2, 130, 59), AttnGrad(2049, 2, 130, 68),
    # columns: H F = 3 (F % 4 is not required), one, two and six column blocks
    AttnGrad(257, 1, 3, 37), AttnGrad(2049, 1, 3, 68), AttnGrad(257, 4, 64, 37), AttnGrad(257, 8, 192, 37),
    AttnGrad(5, 8, 192, 5, pad_y=1, pad_g=1), AttnGrad(1025, 4, 64, 59, pad_y=0, pad_g=0),
)


def attn_grad_inputs(c, kind):
    g = _gen(c.name, kind)
    if kind == "a":
        return {"Y": _ints(g, (c.N, c.HF)), "gelr": _ints(g, (c.N, 2 * c.H))}
    return {"Y": torch.randn((c.N, c.HF), generator=g), "gelr": torch.randn((c.N, 2 * c.H), generator=g)}


def attn_grad_reference(c, Y, gelr):
    """float64 (g [2, HF], den [2, HF])."""
    Y, ge = Y.double(), gelr.double()
    h = torch.arange(c.HF) // c.F
    gl, gr = ge[:, h], ge[:, c.H + h]                     # [N, HF]
    return (torch.stack([(gl * Y).sum(0), (gr * Y).sum(0)]),
            torch.stack([(gl.abs() * Y.abs()).sum(0), (gr.abs() * Y.abs()).sum(0)]))


def attn_grad_emulation(c, Y, gelr):
    """The two kernels in fp32, in their order: per split four fma chains over rows r0 + 4 i + j (the
    tail onto chain 0), (s0 + s1) + (s2 + s3), then the splits in sequence from zero."""
    S, rows_per, _ = attn_grad_plan(c.N, c.HF)
    h = torch.arange(c.HF) // c.F
    tot = torch.zeros((2, c.HF))
    for z in range(S):
        r0, r1 = z * rows_per, min(c.N, (z + 1) * rows_per)
        s = torch.zeros((4, 2, c.HF))
        r = r0
        while r + 4 <= r1:
            for j in range(4):
                gg = torch.stack([gelr[r + j, h], gelr[r + j, c.H + h]])
                s[j] = _fma32(gg, Y[r + j][None], s[j])
            r += 4
        while r < r1:
            gg = torch.stack([gelr[r, h], gelr[r, c.H + h]])
            s[0] = _fma32(gg, Y[r][None], s[0])
            r += 1
        tot = tot + ((s[0] + s[1]) + (s[2] + s[3]))
    return tot


# ====================================================================== 5. head mean
@dataclass(frozen=True)
class HeadMean:
    N: int
    H: int
    F: int
    pad_x: int = 4            # the wide rows' stride: H F + pad_x
    pad_r: int = 8            # the narrow rows' stride: F + pad_r

    @property
    def name(self):
        return f"head_mean/{self.N}/h{self.H}f{self.F}/p{self.pad_x}.{self.pad_r}"


HEAD_MEAN_CASES = tuple(
    [HeadMean(n, h, f) for h in (1, 2, 3, 4, 8) for f in (4, 24, 100) for n in (0, 1, 63, 65, 257)] +
    # the GATv2 call shape: the weight matrix as ONE row of H blocks of F * Fin
    [HeadMean(1, 2, 24 * 75, 0, 0), HeadMean(1, 4, 96 * 768, 4, 4), HeadMean(1, 3, 24 * 75)])


def head_mean_inputs(c, kind):
    """X [N, H F] (kind a: integer multiples of H) and gR [N, F]."""
    g = _gen(c.name, kind)
    if kind == "a":
        return {"X": _ints(g, (c.N, c.H * c.F)) * c.H, "gR": _ints(g, (c.N, c.F)) * c.H}
    return {"X": torch.randn((c.N, c.H * c.F), generator=g), "gR": torch.randn((c.N, c.F), generator=g)}


def head_mean_reference(c, X):
    x = X.double().reshape(c.N, c.H, c.F)
    return x.sum(1) / c.H, x.abs().sum(1) / c.H


def head_mean_emulation(c, X):
    x = X.reshape(c.N, c.H, c.F)
    s = x[:, 0].clone()
    for h in range(1, c.H):
        s = s + x[:, h]
    return s / float(c.H)
