"""Case tables, input makers, the float64 reference and the bars of the GEMM edge tests
(csrc/gemm_f32.hip, gemm_smallk.hip, gemm_prep.hip, gemm_common.h).  No GPU import: the CPU
conditions on these inputs are in test_gemm_cases_cpu.py, the GPU comparisons in
test_gpu_gemm_edges.py.

Every product is C[M][N] = act(A B^T + bias + beta C0) with the LOGICAL operands A [M][K] and
B [N][K]; a case says how they are laid out for the entry point (a_kmajor / b_kmajor, pitches,
base offsets) and which kernel path it is meant to reach (labels).

Two kinds of input per case:
 (a) exact: integers in [-8, 8], every A row times 2^-e (one row all zero).  Every split is then
     exact (split-fp16: the low plane is zero; bf16: <= 4 significant bits) and every partial sum
     is an integer below 2^19 in units of its row's 2^-e, so ANY precision, tile, layout and
     summation order gives the float64 result cast to fp32, bit for bit.  e runs over 0 .. 20;
     0 .. 8 where the entry scales A with one operand-wide power of two; and at most 16 where a
     bias or beta C0 (integers below 2^5) is added, so that unit 2^-16 up to 2^6 still fits in
     24 bits.
 (b) real: randn entries with the same per-row range; the statistic is
         e = max_ij |C_ij - ref_ij| / den_ij,   den = (|A| |B|^T)_ij + |bias_j| + |beta C0_ij|
     in float64 and the bar 3 * 2^-22 + 4 * e_cpu: 2^-22 per operand's representation plus
     2^-22 for the dropped l_a l_b term (gemm_common.h), and e_cpu, the same statistic of
     torch's CPU fp32 product of the same inputs, standing in for the fp32 accumulation.
"""
import zlib
from dataclasses import dataclass

import torch

POISON_BITS = 0x7FC5A5A5      # a quiet NaN with a payload: what every gap and margin holds
BAR_SPLIT = 3 * 2.0 ** -22
ELU_ULP = 2.0 ** -21          # expm1f and the final rounding: 4 ulp of the result
SK_MAX_K = 96                 # gemm_smallk.hip kSkMaxK

# entries whose A is scaled by ONE power of two (the others: a scale per row, or none)
OPERAND_WIDE = ("f16x2", "f16x2_amax", "f16x2_bsplit", "f16x2_batched", "colsum")
KIND_A_ONLY = ("bf16",)


@dataclass(frozen=True)
class Case:
    group: str                # the table (one pytest parameter per group)
    entry: str                # f32 | f32x3 | bf16 | f16x2 | f16x2_amax | f16x2_rows | f16x2_bsplit |
                              # f16x2_ex | f16x2_batched | f32x3_batched | colsum
    M: int
    N: int
    K: int
    ak: int = 0
    bk: int = 0
    opts: tuple = ()          # ((option name, value), ...) for mvml_gat._lib.option
    pad_a: int = 4            # lda = (ak ? M : K) + pad_a, likewise B and C
    pad_b: int = 4
    pad_c: int = 4
    off_a: int = 0            # base offsets in floats past a 16-B aligned address
    off_c: int = 0
    off_bias: int = 0
    bias: bool = False
    beta: float = 0.0
    act: int = 0
    il4: bool = False         # B also given as its il4 image (rows / ex entries)
    batch: int = 1
    kinds: str = "ab"
    labels: tuple = ()
    smallk: int = -1          # expected mvml_gemm_rows_smallk, -1: not asked
    splitk: bool = False      # mvml_gemm_workspace_size must exceed 256
    rows_cols: int = 0        # ex: c_rows_cols
    pad_aux: int = 0          # ex act 3: ld_aux = N + pad_aux
    sum_off: int = 0          # colsum
    sum_n: int = 0
    alpha: float = 1.0
    fused: int = -1           # colsum: expected mvml_gemm_colsum_fused

    @property
    def name(self):
        o = ",".join(f"{k}={v}" for k, v in self.opts)
        return (f"{self.group}/{self.entry}/{self.M}x{self.N}x{self.K}/l{self.ak}{self.bk}/"
                f"p{self.pad_a}.{self.pad_b}.{self.pad_c}/o{self.off_a}.{self.off_c}.{self.off_bias}/"
                f"b{int(self.bias)}{self.beta:g}a{self.act}i{int(self.il4)}z{self.batch}"
                f"r{self.rows_cols}x{self.pad_aux}s{self.sum_off}.{self.sum_n}.{self.alpha:g}/{o}")

    @property
    def lda(self):
        return (self.M if self.ak else self.K) + self.pad_a

    @property
    def ldb(self):
        return (self.N if self.bk else self.K) + self.pad_b

    @property
    def ldc(self):
        return self.N + self.pad_c

    @property
    def emax(self):
        e = 8 if (self.entry in OPERAND_WIDE) else 20
        return min(e, 16) if (self.bias or self.beta != 0.0) else e

    def kind_list(self):
        return [k for k in self.kinds if not (k == "b" and self.entry in KIND_A_ONLY)]


def x3w_fast(c):
    """gemm_f32.hip x3w_fast for a case (bases are 16-B aligned but for off_a)."""
    av = c.lda % 4 == 0 and c.off_a % 4 == 0
    bv = c.ldb % 4 == 0
    return (av and bv and ((c.ak and c.bk) or c.K % 4 == 0) and (not c.ak or c.M % 4 == 0)
            and (not c.bk or c.N % 4 == 0))


def image_ok(c):
    """mvml_split_f16x2_il4 can make B's image: columns and pitch multiples of 4."""
    cols = c.N if c.bk else c.K
    return cols % 4 == 0 and c.ldb % 4 == 0


# ------------------------------------------------------------------------------ tables
def _vary(base, ms, ns, ks):
    """One dimension at a time around base."""
    m0, n0, k0 = base
    out = [base] + [(m, n0, k0) for m in ms] + [(m0, n, k0) for n in ns] + [(m0, n0, k) for k in ks]
    return list(dict.fromkeys(out))


LAYOUTS = ((0, 0), (0, 1), (1, 0), (1, 1))
# one launch (the N split has its own table), and mvml_gemm_f16x2_rows on the tile at any K (the
# small-K kernel has its own table)
T256 = (("gemm_tile", 256), ("gemm_nsplit", 0), ("smallk", 0))
T128 = (("gemm_tile", 128), ("smallk", 0))


def _tile256():
    shapes = _vary((257, 260, 36), (1, 31, 33, 128, 129, 255, 256, 257), (1, 4, 63, 65, 252, 256, 257, 260),
                   (4, 12, 16, 20, 36, 76, 1, 17, 74)) + [(1, 1, 1), (256, 256, 16)]
    out = []
    for entry, il4 in (("f32x3", False), ("f16x2", False), ("f16x2_amax", False), ("f16x2_rows", False),
                       ("f16x2_rows", True), ("f16x2_bsplit", False), ("bf16", False)):
        for ak, bk in LAYOUTS:
            if ak and entry == "f16x2_rows":
                continue
            for m, n, k in shapes:
                c = Case("tile256", entry, m, n, k, ak, bk, opts=T256, il4=il4)
                if (il4 or entry == "f16x2_bsplit") and not image_ok(c):
                    continue
                lab = ["tile256-fast" if x3w_fast(c) else "tile256-guarded"]
                if (ak and m % 4) or (bk and n % 4):
                    lab.append("tile256-kmajor-rows-mod4")
                if (il4 or entry == "f16x2_bsplit") and x3w_fast(c) and not ak:
                    lab.append("tile256-il4")
                out.append(_with(c, labels=tuple(lab)))
    return out


def _with(c, **kw):
    d = {f: getattr(c, f) for f in c.__dataclass_fields__}
    d.update(kw)
    return Case(**d)


def _tile128():
    dims = (1, 63, 65, 127, 128, 129)
    shapes = _vary((129, 129, 36), dims, dims, (4, 31, 32, 33, 36, 74)) + [(128, 128, 32), (1, 1, 4)]
    out = []
    for entry in ("f32", "f32x3", "f16x2", "f16x2_amax", "f16x2_rows"):
        for ak, bk in LAYOUTS:
            if ak and entry == "f16x2_rows":
                continue
            for m, n, k in shapes:
                if entry == "f32":
                    lab = "tile128-f32"
                elif ak and bk:
                    lab = "tile128-fragsplit"
                else:
                    lab = "tile128-x3s-bf16" if entry == "f32x3" else "tile128-x3s-f16"
                out.append(Case("tile128", entry, m, n, k, ak, bk, opts=T128, labels=(lab,)))
    return out


def _align():
    out = []
    variants = (("align-dense", dict(pad_a=0, pad_b=0, pad_c=0)),
                ("align-lda+4", dict(pad_a=4)), ("align-lda+1", dict(pad_a=1)),
                ("align-a-base+1", dict(off_a=1)), ("align-ldc+3", dict(pad_c=3)),
                ("align-ldc+4", dict(pad_c=4)), ("align-c-base+1", dict(off_c=1)),
                ("align-bias-base+1", dict(off_bias=1)), ("align-ldb+1", dict(pad_b=1)))
    for opts, shape, entries in ((T256, (132, 260, 36), ("f32x3", "f16x2_amax", "f16x2_rows", "bf16")),
                                 (T128, (132, 68, 36), ("f32", "f32x3", "f16x2_amax"))):
        for entry in entries:
            for ak, bk in ((0, 0), (1, 1)):
                if ak and entry == "f16x2_rows":
                    continue
                for lab, kw in variants:   # one departure each from the dense, aligned operands
                    kw = dict(dict(pad_a=0, pad_b=0, pad_c=0), **kw)
                    out.append(Case("align", entry, *shape, ak, bk, opts=opts, bias=True, act=1,
                                    labels=(lab, "align-tile%d" % opts[0][1]), **kw))
    return out


def _splitk():
    out = []
    for opts, entries in ((T256, ("f32x3", "f16x2_amax", "bf16")), (T128, ("f32", "f32x3", "f16x2_amax"))):
        for entry in entries:
            for ak, bk in ((1, 1), (0, 0)):
                for m, n, k in ((130, 129, 2068), (128, 124, 2068), (130, 129, 4103)):
                    out.append(Case("splitk", entry, m, n, k, ak, bk, opts=opts, bias=True, beta=1.0,
                                    act=1, splitk=True, labels=("splitk-tile%d" % opts[0][1],)))
    return out


def _nsplit():
    out = []
    for ns in (1, 0):
        # (the second launch must also find its columns of B's il4 image: bsplit, rows with il4)
        for entry, il4 in (("f32x3", False), ("f16x2_amax", False), ("f16x2_rows", False), ("f16x2_rows", True),
                           ("f16x2_bsplit", False)):
            for bk in (1, 0):
                for n in (260, 384, 385):
                    c = Case("nsplit", entry, 257, n, 36, 0, bk, bias=True, beta=1.0, il4=il4,
                             opts=(("gemm_tile", 256), ("gemm_nsplit", ns), ("smallk", 0)),
                             labels=("nsplit-on" if ns else "nsplit-off",))
                    if (il4 or entry == "f16x2_bsplit") and not image_ok(c):
                        continue
                    out.append(c)
    return out


def _persist():
    return [Case("persist", entry, 3 * 256 + 5, 3 * 256 + 4, 36, opts=T256 + (("gemm_persist", p),),
                 bias=True, act=1, kinds="a", labels=("persist-%d" % p,))
            for p in (0, 8) for entry in ("f16x2_amax", "f16x2_rows", "f16x2_bsplit", "f32x3", "bf16")]


def ks16_plan(K):
    """Number of 16-deep k steps of the small-K kernel (1 .. 6)."""
    return (K + 15) // 16


def _smallk():
    shapes = _vary((70, 68, 76), (1, 15, 16, 17, 70), (4, 60, 64, 68, 132), (4, 16, 20, 32, 48, 52, 64, 76, 80, 96))
    sk = (("smallk", 1),)
    out = []
    for il4 in (False, True):
        for m, n, k in shapes:
            lab = ("smallk-plan%d" % ks16_plan(k),) + (("smallk-tail",) if k % 16 else ()) + \
                  (("smallk-il4",) if il4 else ("smallk-fp32b",))
            out.append(Case("smallk", "f16x2_rows", m, n, k, opts=sk, bias=True, act=1, il4=il4,
                            smallk=1, labels=lab))
        out.append(Case("smallk", "f16x2_rows", 70, 68, 76, opts=sk, il4=il4, pad_a=0, pad_b=0, pad_c=0,
                        smallk=1, labels=("smallk-dense",)))
        # the neighbours that must fall to the tile
        nb = dict(opts=sk, bias=True, act=1, il4=il4, smallk=0, labels=("smallk-neighbour",))
        out.append(Case("smallk", "f16x2_rows", 70, 68, 100, **nb))
        if not il4:
            out.append(Case("smallk", "f16x2_rows", 70, 70, 76, **nb))
        out.append(Case("smallk", "f16x2_rows", 70, 68, 76, pad_c=1, **nb))
        out.append(Case("smallk", "f16x2_rows", 70, 68, 76, beta=1.0, **nb))
    return out


def _ex():
    out = []
    for act in (0, 1, 2, 3):
        for m in (1, 257):
            for n in (4, 68, 260):
                for k in (20, 76):
                    for bk, il4 in ((0, False), (1, False), (0, True)):
                        out.append(Case("ex", "f16x2_ex", m, n, k, 0, bk, il4=il4, bias=act != 3, act=act,
                                        labels=("ex-act%d" % act, "ex-il4" if il4 else "ex-bk%d" % bk)))
    for bk, il4 in ((0, False), (1, False), (0, True)):
        out.append(Case("ex", "f16x2_ex", 257, 132, 20, 0, bk, il4=il4, bias=True, act=2, rows_cols=64,
                        labels=("ex-rows-cols64",)))
        out.append(Case("ex", "f16x2_ex", 257, 260, 20, 0, bk, il4=il4, bias=True, act=2, rows_cols=256,
                        labels=("ex-rows-cols256",)))
        for act in (2, 3):
            out.append(Case("ex", "f16x2_ex", 257, 68, 20, 0, bk, il4=il4, bias=act != 3, act=act, batch=2,
                            labels=("ex-batch2",)))
        out.append(Case("ex", "f16x2_ex", 257, 132, 20, 0, bk, il4=il4, bias=True, act=1, batch=2,
                        rows_cols=64, labels=("ex-batch2", "ex-rows-cols64")))
        out.append(Case("ex", "f16x2_ex", 257, 68, 76, 0, bk, il4=il4, act=3, pad_aux=1,
                        labels=("ex-aux-unaligned",)))
        out.append(Case("ex", "f16x2_ex", 257, 68, 76, 0, bk, il4=il4, act=3, pad_aux=4,
                        labels=("ex-aux-pitched",)))
    return out


def _batched():
    out = []
    for entry in ("f16x2_batched", "f32x3_batched"):
        x3 = entry == "f32x3_batched"
        for opts in (T256, T128):
            for ak, bk in LAYOUTS:
                for m, n, k in ((100, 70, 36), (257, 130, 20)):
                    out.append(Case("batched", entry, m, n, k, ak, bk, opts=opts, batch=3, bias=x3,
                                    beta=1.0 if x3 else 0.0,
                                    labels=("batched-f32x3" if x3 else "batched-f16x2",)))
    return out


def _colsum():
    out = []
    for (m, n, k), pa, so, sn, al in (((130, 20, 100), 7, 0, 130, 1.0), ((132, 20, 100), 8, 30, 64, 0.25),
                                      ((129, 76, 36), 7, 65, 64, 1.0), ((129, 76, 36), 3, 0, 1, 0.25)):
        out.append(Case("colsum", "colsum", m, n, k, 1, 1, pad_a=pa, pad_b=0, sum_off=so, sum_n=sn, alpha=al,
                        fused=1, labels=("colsum-fused",)))
    out.append(Case("colsum", "colsum", 130, 20, 2068, 1, 1, pad_a=6, sum_off=2, sum_n=128, alpha=0.25,
                    fused=1, splitk=True, labels=("colsum-fused-splitk",)))
    # N = 100 alone still takes the skinny (fused) plan; forced to the 256x256 tile it is the
    # product followed by mvml_colsum_f32
    out.append(Case("colsum", "colsum", 130, 100, 36, 1, 1, pad_a=6, sum_off=30, sum_n=100, alpha=1.0,
                    fused=1, labels=("colsum-fused",)))
    out.append(Case("colsum", "colsum", 130, 100, 36, 1, 1, opts=T256, pad_a=6, sum_off=30, sum_n=100,
                    alpha=0.25, fused=0, labels=("colsum-unfused",)))
    return out


TABLES = {"tile256": _tile256, "tile128": _tile128, "align": _align, "splitk": _splitk, "nsplit": _nsplit,
          "persist": _persist, "smallk": _smallk, "ex": _ex, "batched": _batched, "colsum": _colsum}
CASES = [c for t in TABLES.values() for c in t()]

REQUIRED_LABELS = (
    "tile256-fast", "tile256-guarded", "tile256-kmajor-rows-mod4", "tile256-il4",
    "tile128-f32", "tile128-x3s-bf16", "tile128-x3s-f16", "tile128-fragsplit",
    "align-dense", "align-lda+4", "align-lda+1", "align-a-base+1", "align-ldc+3", "align-ldc+4",
    "align-c-base+1", "align-bias-base+1", "align-tile256", "align-tile128",
    "splitk-tile256", "splitk-tile128", "nsplit-on", "nsplit-off", "persist-0", "persist-8",
    "smallk-plan1", "smallk-plan2", "smallk-plan3", "smallk-plan4", "smallk-plan5", "smallk-plan6",
    "smallk-tail", "smallk-il4", "smallk-fp32b", "smallk-neighbour",
    "ex-act0", "ex-act1", "ex-act2", "ex-act3", "ex-bk0", "ex-bk1", "ex-il4", "ex-rows-cols64",
    "ex-rows-cols256", "ex-batch2", "ex-aux-unaligned",
    "batched-f16x2", "batched-f32x3", "colsum-fused", "colsum-fused-splitk", "colsum-unfused",
)


def groups():
    """{(table, entry, layout): [cases]}: one pytest parameter each."""
    out = {}
    for c in CASES:
        out.setdefault(f"{c.group}-{c.entry}-{c.ak}{c.bk}", []).append(c)
    return out


def all_ks():
    return sorted({c.K for c in CASES})


# ------------------------------------------------------------------------------ inputs
def _gen(c, kind):
    return torch.Generator().manual_seed(zlib.crc32((c.name + kind).encode()))


def make_inputs(c, kind):
    """CPU fp32 tensors of the logical operands: A [batch, M, K], B [batch, N, K], bias
    [batch or 1, N] | None (only mvml_gemm_f16x2_ex strides its bias), C0 [batch, M, N] | None,
    aux [1, M, N] | None (act 3; shared by the products of a batch)."""
    g = _gen(c, kind)
    z, M, N, K = c.batch, c.M, c.N, c.K
    e = torch.randint(0, c.emax + 1, (z, M, 1), generator=g)
    if M >= 2:
        e[:, 0], e[:, M - 1] = 0, c.emax   # both ends of the range in every product
    scale = torch.pow(2.0, -e.float())
    zb = z if c.entry == "f16x2_ex" else 1
    if kind == "a":
        A = torch.randint(-8, 9, (z, M, K), generator=g).float() * scale
        if M >= 3:
            A[:, M // 2] = 0.0             # max |row| = 0: the clamped amax_shift
        B = torch.randint(-8, 9, (z, N, K), generator=g).float()
        bias = torch.randint(-8, 9, (zb, N), generator=g).float() if c.bias else None
        C0 = torch.randint(-8, 9, (z, M, N), generator=g).float() if c.beta != 0.0 else None
        # aux + 1 in {0, 1/2, 1}: the ELU' factor is a power of two or zero
        aux = torch.tensor([-1.0, -0.5, 0.0, 1.0, 2.5])[torch.randint(0, 5, (1, M, N), generator=g)]
    else:
        A = torch.randn((z, M, K), generator=g) * scale
        B = torch.randn((z, N, K), generator=g)
        bias = torch.randn((zb, N), generator=g) if c.bias else None
        C0 = torch.randn((z, M, N), generator=g) if c.beta != 0.0 else None
        aux = torch.nn.functional.elu(torch.randn((1, M, N), generator=g))   # a layer output: > -1
    return {"A": A, "B": B, "bias": bias, "C0": C0, "aux": aux if c.act == 3 else None}


def _act(c, pre, aux, dtype):
    if c.act == 1:
        return pre.clamp_min(0.0)
    if c.act == 2:
        return torch.where(pre > 0, pre, torch.expm1(pre))
    if c.act == 3:
        a = aux.to(dtype)
        return pre * torch.where(a > 0, torch.ones_like(a), a + 1.0)
    return pre


def _product(c, inp, dtype):
    pre = inp["A"].to(dtype) @ inp["B"].to(dtype).transpose(1, 2)
    if inp["bias"] is not None:
        pre = pre + inp["bias"].to(dtype)[:, None, :]
    if inp["C0"] is not None:
        pre = pre + c.beta * inp["C0"].to(dtype)
    return pre


def reference(c, inp):
    """float64: (ref after the activation, pre-activation, den) each [batch, M, N]."""
    pre = _product(c, inp, torch.float64)
    den = inp["A"].double().abs() @ inp["B"].double().abs().transpose(1, 2)
    if inp["bias"] is not None:
        den = den + inp["bias"].double().abs()[:, None, :]
    if inp["C0"] is not None:
        den = den + abs(c.beta) * inp["C0"].double().abs()
    return _act(c, pre, inp["aux"], torch.float64), pre, den


def cpu_fp32_pre(c, inp):
    """torch's CPU fp32 product + bias + beta C0 (before the activation): a reference."""
    return _product(c, inp, torch.float32)


def stat(x, ref, den):
    """max |x - ref| / den over den > 0 (where den == 0 the result must be exactly ref)."""
    d = (x.double() - ref).abs()
    ok = den > 0
    if bool((d[~ok] != 0).any()):
        return float("inf")
    return (d[ok] / den[ok]).max().item() if bool(ok.any()) else 0.0


def bar(e_cpu):
    return BAR_SPLIT + 4.0 * e_cpu


def colsum_reference(c, inp):
    """float64 alpha * sum_k A[sum_off + j][k] and the sum of absolute values, j < sum_n."""
    rows = inp["A"][0, c.sum_off:c.sum_off + c.sum_n].double()
    return c.alpha * rows.sum(1), c.alpha * rows.abs().sum(1)


def first_diff(x, ref):
    """(count, index tuple of the first element) where two equal-shape tensors differ in value
    (a NaN differs from everything)."""
    ne = x != ref
    idx = ne.nonzero()
    return int(idx.shape[0]), (tuple(idx[0].tolist()) if idx.shape[0] else None)


# ------------------------------------------------------------------------------ split emulation
def amax_shift(maxabs):
    """gemm_common.h amax_shift of a float tensor of maxima: 141 - biased exponent, clamped."""
    bits = maxabs.float().contiguous().view(torch.int32)
    return (141 - ((bits >> 23) & 0xFF)).clamp(-100, 100)


def split2h(x, shift):
    """gemm_common.h split2h: x 2^shift = h + l in fp16 (fp32 tensors of the two planes)."""
    xs = x.float() * torch.pow(2.0, shift.float())
    h = xs.half().float()
    l = (xs - h).half().float()
    return h, l


def a_shift(c, A):
    """The scale shift of every A row [batch, M, 1] as the entry derives it."""
    if c.entry in OPERAND_WIDE:
        return amax_shift(A.abs().max()).expand(A.shape[0], A.shape[1], 1)
    return amax_shift(A.abs().amax(2, keepdim=True))


def emulate_split(A, B, sa, sb, drop=False):
    """The split-fp16 product h_a h_b + h_a l_b + l_a h_b (fp32 accumulation on the CPU), scaled
    back; drop = True leaves out l_a h_b (the mutation the bar must catch)."""
    ha, la = split2h(A, sa)
    hb, lb = split2h(B, sb)
    bt = hb.transpose(-1, -2)
    acc = ha @ bt + ha @ lb.transpose(-1, -2)
    if not drop:
        acc = acc + la @ bt
    return acc.double() * torch.pow(2.0, -(sa + sb).double())
