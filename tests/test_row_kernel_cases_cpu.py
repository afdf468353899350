"""CPU conditions on _row_kernel_cases.py (no GPU): what test_gpu_row_kernels.py relies on.

 a. every float64 restatement agrees with an independent one to 1e-12 relative (the oracle's
    GraphNorm and its autograd, F.layer_norm, torch.softmax autograd, F.binary_cross_entropy_with_logits,
    torch.optim.Adam(foreach=False) in float64);
 b. the tables reach every kernel instance, slot count, reduction regime and sweep the GPU file names;
 c. the reference alone stays inside each bar: the same formulas in float32 on the CPU pass the fp32
    kernels' checks, an fp64 evaluation in the kernel's own sequential order rounded to fp32 passes
    GraphNorm's (and an fp32 evaluation of GraphNorm does NOT on x + 1000: the bar sees fp32 statistics);
 d. the special patterns are what they claim;
 e. every refusal added to the entries returns MVML_ERR_INVALID / MVML_ERR_WORKSPACE and names its
    entry, without a GPU (a refused call returns before it touches the runtime).
"""
import ctypes

import pytest
import torch
import torch.nn.functional as F

import _row_kernel_cases as R
from mvml_gat import _lib
from oracle import gnn_ref

F64, F32 = torch.float64, torch.float32


def _close(a, b, what):
    scale = max(float(b.abs().max()), 1e-300) if b.numel() else 1.0
    assert float((a - b).abs().max() if b.numel() else 0.0) <= 1e-12 * scale, what


# ------------------------------------------------------------------ a. independent references
@pytest.mark.parametrize("c", [c for c in R.GN_CASES if c.D <= 257 and c.xpat != "offset"][::3], ids=lambda c: c.name)
def test_graphnorm_reference_vs_oracle(c):
    inp = R.gn_inputs(c)
    x, w, b, ms = (inp[k].double().requires_grad_() for k in ("x", "w", "b", "ms"))
    # (the oracle takes the mean of every group it is given: the same rows without the empty groups)
    y = gnn_ref.graphnorm_ref(x, w, b, ms, R.EPS32, sorted(set(inp["off"])))
    y.backward(inp["gy"].double())
    got = R.gn_eval(inp)
    for g, r, n in zip(got, (y.detach(), x.grad, w.grad, b.grad, ms.grad), ("y", "g_x", "g_w", "g_b", "g_ms")):
        _close(g, r, (c.name, n))


@pytest.mark.parametrize("c", R.LN_CASES[::4], ids=lambda c: c.name)
def test_layernorm_reference_vs_torch(c):
    inp = R.ln_inputs(c)
    x, gm, bt = (inp[k].double().requires_grad_() for k in ("x", "gamma", "beta"))
    y = F.layer_norm(x, (c.D,), gm, bt, R.EPS32)
    y.backward(inp["gy"].double())
    yr, mean, rstd = R.ln_fwd(inp)
    gx, gyxh = R.ln_bwd(inp, mean=mean, rstd=rstd)          # the exact statistics, not their fp32 values
    _close(yr, y.detach(), c.name)
    # var = 0 rows: g_x is a cancelling sum scaled by 1 / sqrt(eps); relative to its den instead
    assert ((gx - x.grad).abs() <= 1e-12 * R.ln_bwd(inp, absolute=True)[0]).all(), c.name
    assert ((gyxh.sum(0) - gm.grad).abs() <= 1e-12 * R.ln_bwd(inp, absolute=True)[1].sum(0)).all(), c.name
    _close(inp["gy"].double().sum(0), bt.grad, c.name)


@pytest.mark.parametrize("c", [c for c in R.AT_CASES if c.pat != "saturated"][::3], ids=lambda c: c.name)
def test_attention_reference_vs_softmax_autograd(c):
    inp = R.at_inputs(c)
    qkv = inp["qkv"].double().requires_grad_()
    t = qkv.reshape(c.B, 3, 3, c.H, c.dk).permute(2, 0, 3, 1, 4)
    P = torch.softmax(t[0] @ t[1].transpose(-1, -2) * inp["scale"], -1)
    att = P @ t[2]
    att.backward(inp["g_att"].double())
    a, Pr = R.at_fwd(c, inp)
    _close(a, att.detach(), c.name)
    _close(Pr, P.detach(), c.name)
    _close(R.at_bwd(c, inp, P=Pr), qkv.grad, c.name)


@pytest.mark.parametrize("c", R.BCE_CASES, ids=lambda c: c.name)
def test_bce_reference_vs_torch(c):
    inp = R.bce_inputs(c)
    z = inp["z"].double().requires_grad_()
    terms = F.binary_cross_entropy_with_logits(z, inp["y"].double(), reduction="none")
    terms.mean().backward()
    lt, gz = R.bce_eval(inp)
    # (torch forms (1 - y) z + m + log(exp(-m) + exp(-z - m)), m = max(-z, 0): at z = -89, y = 0 that is
    # -89 + 89 + log(1 + 2e-39) = 0, so it is itself only good to a few 2^-53 (1 + |z|) absolute)
    slack = 4 * 2.0 ** -53 * (1 + inp["z"].double().abs())
    assert ((lt - terms.detach()).abs() <= 1e-12 * R.bce_eval(inp, absolute=True)[0] + slack).all(), c.name
    _close(gz, z.grad, c.name)


@pytest.mark.parametrize("betas,wd", [((0.9, 0.999), 1e-4), ((0.0, 0.0), 0.0), ((0.9, 0.999), 0.0)])
def test_adam_reference_vs_torch(betas, wd):
    """Three steps of torch.optim.Adam(foreach=False) in float64; the middle parameter never has a
    gradient and must keep its value, moments and step."""
    c = R.OPT("p3b", 100, wd, 1.0, betas)
    g = torch.Generator().manual_seed(5)
    ps = [torch.randn(n, generator=g, dtype=F64).requires_grad_() for n in (7, 5, 300)]
    opt = torch.optim.Adam(ps, lr=c.lr, betas=betas, eps=c.eps, weight_decay=wd, foreach=False)
    mine = [{"p": p.detach().clone(), "m": torch.zeros_like(p), "v": torch.zeros_like(p), "step": 0} for p in ps]
    for _ in range(3):
        for i, (p, q) in enumerate(zip(ps, mine)):
            p.grad = None if i == 1 else torch.randn(p.shape, generator=g, dtype=F64)
            if i != 1:
                q["g"] = p.grad.clone()
                q["p"], q["m"], q["v"] = R.adam_eval(c, q)
                q["step"] += 1
        opt.step()
    for i, (p, q) in enumerate(zip(ps, mine)):
        _close(q["p"], p.detach(), i)
        if i == 1:
            assert p not in opt.state or not opt.state[p]
            assert q["step"] == 0 and not q["m"].any()
        else:
            _close(q["m"], opt.state[p]["exp_avg"], i)
            _close(q["v"], opt.state[p]["exp_avg_sq"], i)
            assert int(opt.state[p]["step"]) == q["step"] == 3


# ------------------------------------------------------------------ b. what the tables reach
def test_graphnorm_table():
    assert {c.D for c in R.GN_CASES} == set(R.GN_D) and {c.G for c in R.GN_CASES} == set(R.GN_G)
    assert {c.grid_y for c in R.GN_CASES} == {1, 2, 3}
    assert [R.gn_regime(g) for g in (48, 49, 63, 64, 112, 113)] == ["tail", "partial", "partial", "all", "all", "two"]
    for regime in ("tail", "partial", "all", "two"):       # each with a D that is not a multiple of 16
        assert any(R.gn_regime(c.G) == regime and c.D % 16 for c in R.GN_CASES), regime
    assert {(c.xpat, c.mspat) for c in R.GN_CASES} == set(R.GN_PATTERNS)
    seen = set()
    for c in R.GN_CASES:
        s = R.gn_sizes(c)
        assert len(s) == c.G and set(s) <= set(R.GN_SIZES) and sum(s) > 0, c.name
        seen |= set(s)
        if c.G >= 4:
            assert s[0] == 0 and s[c.G // 2] == 0 and s[-1] == 0, c.name
        if c.D >= 2:
            assert (R.gn_inputs(c)["w"] == 0).sum() == 1
    assert seen == set(R.GN_SIZES)
    assert len({c.name for c in R.GN_CASES}) == len(R.GN_CASES)


def test_layernorm_table():
    assert {c.D for c in R.LN_CASES} >= set(R.LN_D) and {c.rows for c in R.LN_CASES} == set(R.LN_ROWS)
    for s in range(1, 9):                                   # every slot count, last slot full and partly masked
        assert any(c.slots == s and c.D % 64 == 0 for c in R.LN_CASES), s
        assert any(c.slots == s and c.D % 64 for c in R.LN_CASES), s
    assert {c.rows % 4 for c in R.LN_CASES} >= {0, 1, 3}   # the last workgroup's live waves
    for i in range(4):
        assert any(c.ld(i) == c.D + 1 for c in R.LN_CASES) and any(c.ld(i) == 3 * c.D for c in R.LN_CASES)
        assert any(c.ld(i) == c.D for c in R.LN_CASES)
    assert {c.pat for c in R.LN_CASES} == set(R.LN_PATTERNS)
    assert {c.pat for c in R.LN_CASES if c.D > 384} == set(R.LN_PATTERNS)
    assert len({c.name for c in R.LN_CASES}) == len(R.LN_CASES)


def test_attention_table():
    inst = {R.by_width(c.dk) for c in R.AT_CASES}
    assert inst == {(True, k) for k in range(1, 7)} | {(False, 6)}
    assert {c.dk for c in R.AT_CASES} == set(R.AT_DK) and all(c.dk % 4 == 0 for c in R.AT_CASES)
    assert {c.H for c in R.AT_CASES} == {1, 3, 12} and {c.B for c in R.AT_CASES} == {1, 2, 5}
    assert {c.B * c.H % 4 for c in R.AT_CASES} == {0, 1, 2, 3}
    assert {c.pad for c in R.AT_CASES} == {0, 4} == {c.padg for c in R.AT_CASES}
    for dk in R.AT_DK:
        assert {c.pat for c in R.AT_CASES if c.dk == dk} == set(R.AT_PATTERNS)


def test_elementwise_and_optimizer_tables():
    assert max(R.RELU_N) > R.RELU_GRID_CAP and max(R.RELU_N) * 4 < 17 * 2 ** 20     # one second sweep, 16 MB
    inp = R.relu_inputs(257)
    y = inp["y"]
    assert bool(torch.isnan(y).any()) and bool((y == R.DENORMAL).any()) and R.DENORMAL < 2.0 ** -126
    assert bool(((y == 0) & torch.signbit(y)).any()) and bool(((y == 0) & ~torch.signbit(y)).any())
    ex = R.relu_expected(inp, 2.0)
    assert not torch.isnan(ex).any() and bool((ex[torch.isnan(y)] == 0).all())
    assert R.RELU_SCALES[2] == float(torch.tensor(1 / 0.7, dtype=F32))
    assert {c.P for c in R.OPT_CASES} == {1, 3, 300} and max(c.P for c in R.OPT_CASES) > 256
    assert {c.chunk for c in R.OPT_CASES} == set(R.OPT_CHUNKS)
    assert {(c.wd, c.gs, c.betas) for c in R.OPT_CASES} == set(R.OPT_HYPER)
    sizes, flags, steps = set(), set(), set()
    for c in R.OPT_CASES:
        cp, cb, ce, off, numel = R.opt_tables(c.sizes, c.chunk)
        assert R.tables_ok(c.sizes, cp, cb, ce, off, numel), c.name
        sizes |= set(c.sizes)
        if c.P == 300:
            ps = R.opt_inputs(c)
            flags |= {q["flag"] for q in ps}
            steps |= {q["step"] for q in ps}
            assert any(q["flag"] == 0 and q["p"].numel() > 16384 for q in ps)       # skipped in every chunk
            assert all((q["step"] == 0) == (not q["m"].any() and not q["v"].any()) or q["p"].numel() == 0 for q in ps)
    assert sizes == set(R.OPT_SIZES) and flags == {0.0, 1.0, 2.0} and steps == set(R.OPT_STEPS)
    # the checker itself refuses a straddling chunk, a hole and a misaligned segment
    assert not R.tables_ok((5, 5), [0], [0], [13], [0, 8])
    assert not R.tables_ok((5,), [0], [0], [4], [0])
    assert not R.tables_ok((5, 5), [0, 1], [0, 6], [5, 11], [0, 6])


# ------------------------------------------------------------------ c. the reference alone is inside the bars
def _gn_sequential(inp):
    """norm.hip's kernels in fp64 in their own order (rows in sequence per column; group partials by
    stripe as graphnorm_param_reduce adds them), outputs rounded to fp32."""
    x, w, b, ms, gy = (inp[k].double() for k in ("x", "w", "b", "ms", "gy"))
    D, off = x.shape[1], inp["off"]
    G = len(off) - 1
    y, gx = torch.zeros_like(x), torch.zeros_like(x)
    part = torch.zeros(3, G, D, dtype=F64)
    for gi, (a, e) in enumerate(zip(off[:-1], off[1:])):
        n = e - a
        if n == 0:
            continue
        s = torch.zeros(D, dtype=F64)
        for r in range(a, e):
            s = s + x[r]
        mean = s / n
        v, so, sgy, sgyo = (torch.zeros(D, dtype=F64) for _ in range(4))
        for r in range(a, e):
            o = x[r] - mean * ms
            v, so, sgy, sgyo = v + o * o, so + o, sgy + gy[r], sgyo + gy[r] * o
        var = v / n + R.EPS32
        inv = 1.0 / var.sqrt()
        k = w / (v / n + R.EPS32).sqrt()
        k1, k2 = w * inv, sgyo / (n * var)
        sum_go = k1 * (sgy - k2 * so)
        for r in range(a, e):
            o = x[r] - mean * ms
            y[r] = k * o + b
            gx[r] = k1 * (gy[r] - k2 * o) - ms * sum_go / n
        part[0, gi], part[1, gi], part[2, gi] = sgyo * inv, sgy, -mean * sum_go
    red = torch.zeros(3, 16, D, dtype=F64)
    for stripe in range(16):
        for g in range(stripe, G, 16):
            red[:, stripe] += part[:, g]
    h = 8
    while h:
        red[:, :h] += red[:, h:2 * h]
        h //= 2
    return [t.float() for t in (y, gx, red[0, 0], red[1, 0], red[2, 0])]


@pytest.mark.parametrize("c", [c for c in R.GN_CASES if c.D <= 257], ids=lambda c: c.name)
def test_graphnorm_bar_holds_fp64_and_sees_fp32(c):
    inp = R.gn_inputs(c)
    refs, dens = R.gn_eval(inp), R.gn_eval(inp, absolute=True)
    allowed = R.gn_bars(c, inp, refs, dens)
    for got, r, a, n in zip(_gn_sequential(inp), refs, allowed, ("y", "g_x", "g_w", "g_b", "g_ms")):
        rec, ok = R.allowed_check(got, r, a)
        assert ok, (c.name, n, rec)
    if c.xpat == "offset" and c.mspat == "one":             # fp32 statistics: far outside
        y32 = R.gn_eval(inp, F32)[0]
        assert R.allowed_check(y32, refs[0], allowed[0])[0]["ratio"] > 100, c.name


def test_fp32_references_inside_their_bars():
    """r32 against ref under fp32_check (e32 <= max(4 e32, 8 u) by construction; what this pins is
    that every den is positive where the reference is not exact and every e32 is finite and small)."""
    worst = {}

    def hold(kernel, name, r32, ref, den):
        assert torch.isfinite(ref).all() and torch.isfinite(den).all() and torch.isfinite(r32).all(), name
        rec, ok = R.fp32_check(r32, ref, den, r32)
        assert ok and rec["bar_floor"] < 2e-5, (name, rec)
        worst[kernel] = max(worst.get(kernel, 0.0), rec["bar_floor"])

    for c in R.LN_CASES:
        inp = R.ln_inputs(c)
        for n, r32, ref, den in zip(("y", "mean", "rstd"), R.ln_fwd(inp, F32), R.ln_fwd(inp), R.ln_fwd(inp, absolute=True)):
            hold("layernorm_fwd", c.name + n, r32, ref, den)
        for n, r32, ref, den in zip(("g_x", "g_y_xhat"), R.ln_bwd(inp, F32), R.ln_bwd(inp), R.ln_bwd(inp, absolute=True)):
            hold("layernorm_bwd", c.name + n, r32, ref, den)
    for c in R.AT_CASES:
        inp = R.at_inputs(c)
        for n, r32, ref, den in zip(("att", "P"), R.at_fwd(c, inp, F32), R.at_fwd(c, inp), R.at_fwd(c, inp, absolute=True)):
            hold("token_attn_fwd", c.name + n, r32, ref, den)
        hold("token_attn_bwd", c.name, R.at_bwd(c, inp, F32), R.at_bwd(c, inp), R.at_bwd(c, inp, absolute=True))
    for c in R.BCE_CASES:
        inp = R.bce_inputs(c)
        for n, r32, ref, den in zip(("loss", "g_z"), R.bce_eval(inp, F32), R.bce_eval(inp), R.bce_eval(inp, absolute=True)):
            hold("bce_logits", c.name + n, r32, ref, den)
    for c in R.OPT_CASES:
        for q in R.opt_inputs(c):
            for n, r32, ref, den in zip("pmv", R.adam_eval(c, q, F32), R.adam_eval(c, q), R.adam_eval(c, q, absolute=True)):
                hold("adam_flat", c.name + n, r32, ref, den)
    print("largest floor-adjusted bar per kernel:", {k: f"{v:.2e}" for k, v in worst.items()})


def test_bitwise_expectations():
    for n in R.RELU_N[:4]:
        inp = R.relu_inputs(n)
        for s in R.RELU_SCALES:
            ex = R.relu_expected(inp, s)
            want = torch.where(inp["y"].double() > 0, (inp["gy"].double() * s), torch.zeros(n, dtype=F64)).float()
            assert torch.equal(ex, want) and not torch.signbit(ex[~(inp["y"] > 0)]).any()


# ------------------------------------------------------------------ d. the special patterns
def test_saturated_attention_underflows_and_stays_finite():
    for c in R.AT_CASES:
        if c.pat != "saturated":
            continue
        inp = R.at_inputs(c)
        att, P = R.at_fwd(c, inp)
        assert bool(((P > 0) & (P < 2.0 ** -149)).any()), c.name
        assert ((P.max(-1).values > 1 - 1e-12)).all(), c.name
        assert (inp["P32"] == 0).sum() == 6 * c.B * c.H, c.name     # two of three underflow in fp32
        g = R.at_bwd(c, inp)
        assert torch.isfinite(g).all() and torch.isfinite(att).all() and bool(g.abs().max() > 0), c.name
        s = (lambda q, k: (q @ k.transpose(-1, -2)) * inp["scale"])(*R._qkv(c, inp, F64)[:2])
        top = s.sort(-1).values
        assert ((top[..., 2] - top[..., 1]) > 110).all(), c.name


def test_equal_attention_has_nine_equal_scores():
    for c in R.AT_CASES:
        if c.pat == "equal":
            inp = R.at_inputs(c)
            assert torch.equal(R.at_fwd(c, inp, F32)[1], torch.full((c.B, c.H, 3, 3), 1 / 3, dtype=F32)), c.name


def test_const_patterns_have_zero_variance():
    for c in R.GN_CASES:
        if c.xpat == "const":
            inp = R.gn_inputs(c)
            x = inp["x"].double()
            for a, e in zip(inp["off"][:-1], inp["off"][1:]):
                if e > a:
                    assert not (x[a:e] - x[a:e].sum(0) / (e - a)).any(), c.name
            assert bool((inp["ms"] == 1).all())
            assert torch.equal(R.gn_eval(inp)[0], inp["b"].double().expand_as(x)), c.name     # eps decides: y = bias
    for c in R.LN_CASES:
        if c.pat == "const":
            x = R.ln_inputs(c)["x"].double()
            assert not (x[0] - x[0].sum() / c.D).any(), c.name


def test_planted_bce_logits_give_finite_fp32_terms():
    for c in R.BCE_CASES:
        inp = R.bce_inputs(c)
        if c.n > 1:
            assert set(torch.tensor(R.BCE_PLANTED, dtype=F32).tolist()) <= set(inp["z"].tolist())
            assert 0.0 <= float(inp["y"].min()) and float(inp["y"].max()) <= 1.0
            assert c.soft == bool(((inp["y"] > 0) & (inp["y"] < 1)).any())
        lt, gz = R.bce_eval(inp, F32)
        assert torch.isfinite(lt).all() and torch.isfinite(gz).all(), c.name


# ------------------------------------------------------------------ e. the refusals, without a GPU
# a non-NULL, 16-byte aligned value that a refused call never follows, and one 4 bytes past it
REFUSALS = R.refusals(ctypes.c_void_p(4096), ctypes.c_void_p(4100))


@pytest.mark.parametrize("what", list(REFUSALS))
def test_refusals_without_gpu(what):
    entry, who, code, args = REFUSALS[what]
    L = _lib.lib()
    rc = getattr(L, entry)(*args)
    msg = L.mvml_last_error().decode(errors="replace")
    assert rc == code, (rc, msg)
    assert who in msg, msg


def test_refusal_table_names_every_pointer():
    protos = _lib.parse_header()
    for entry in {v[0] for v in REFUSALS.values()}:
        n_ptr = sum(1 for a in protos[entry][1] if a is ctypes.c_void_p) - 1          # all but the stream
        optional = 3 if entry == "mvml_graphnorm_bwd" else 0                          # the three parameter gradients
        assert sum(1 for k in REFUSALS if k.startswith(entry + ":") and k.endswith(" NULL")) == n_ptr - optional, entry
