"""CPU conditions on the GAT parameter-side cases of _gat_param_cases.py (no GPU): what
test_gpu_gat_params.py relies on must hold for every case in the tables.

 1. kind (a) inputs are exact: every operand survives the bf16 and the scaled split-fp16 split
    unchanged, every sum of absolute terms stays below 2^24 in units of its row's 2^-e, and an fp32
    evaluation in any order reproduces the float64 reference bit for bit;
 2. the projection table reaches all 32 kernel instances that carry the logit epilogue (and the
    f16x2 fallback at tile 128), at the rows, K and widths of the table;
 3. the fold reference is linear and the unfold reference is its adjoint;
 4. the attention-vector gradient equals its re-associated form (GATLayerFunction.backward);
 5. an fp32 emulation of every helper kernel, in the kernel's own order, stays inside its bar, so
    the bars cannot fail a correct kernel.
"""
import pytest
import torch

import _gat_param_cases as P
import _gemm_cases as G

PROJ_GROUPS = P.proj_groups()


# ------------------------------------------------------------------ 1. exactness of kind (a)
@pytest.mark.parametrize("group", sorted(PROJ_GROUPS))
def test_proj_exact_inputs_are_exact(group):
    for c in PROJ_GROUPS[group] + (list(P.PROJ_MAXIMA) if group == "f16x2-t256" else []):
        inp = P.proj_inputs(c, "a")
        X, W, a = inp["X"], inp["W"], inp["a"]
        for t in (X, W, a):
            assert torch.equal(t.bfloat16().float(), t), c.name       # <= 4 significant bits
        # the split-fp16 planes: X at ONE operand-wide scale, Wcat likewise; the low planes are zero
        _, lx = P.split2h(X, P.amax_shift(X.abs().max()))
        _, lw = P.split2h(W, P.amax_shift(W.abs().max()))
        if c.algo == "f16x2":
            assert not lx.any() and not lw.any(), c.name
        assert c.emax == (8 if c.algo == "f16x2" else 20), c.name
        Y, elr, den_y, den_el = P.proj_reference(c, inp)
        unit = torch.pow(2.0, inp["e"].double())[:, None]              # 1 / the row's 2^-e
        assert (den_y * unit).max() < 2 ** 24 and (den_el * unit).max() < 2 ** 24, c.name
        assert torch.equal(Y * unit, (Y * unit).round()) and torch.equal(elr * unit, (elr * unit).round()), c.name
        if c.N >= 3:
            assert not X[c.N // 2].any(), c.name                       # the all-zero row
        y32, el32 = P.proj_cpu_fp32(c, inp)
        assert torch.equal(y32.double(), Y) and torch.equal(el32.double(), elr), c.name
        assert torch.equal(P.proj_epilogue_emulation(c, y32, a).double(), elr), c.name
        assert c.attn_lim == 8 or c.K * c.F > 7600, c.name


def test_helper_exact_inputs_are_exact():
    for c in P.FOLD_CASES:
        inp = P.fold_inputs(c, "a")
        ref, den = P.fold_reference(c, inp["fc"], inp["res"], inp["a"])
        assert den.max() < 2 ** 24 and torch.equal(ref, ref.round()), c.name
        assert torch.equal(P.fold_emulation(c, inp["fc"], inp["res"], inp["a"]).double(), ref), c.name
        un = P.unfold_inputs(c, "a")
        g_fc, g_res, den = P.unfold_reference(c, un["gW"], un["a"])
        assert den.max() < 2 ** 24 and torch.equal(g_fc, g_fc.round()), c.name
        assert g_res is None or torch.equal(g_res, g_res.round()), c.name
        assert torch.equal(P.unfold_emulation(c, un["gW"], un["a"]).double(), g_fc), c.name
    for c in P.ATTN_GRAD_CASES:
        assert c.N <= 2 ** 18, c.name                                  # N * 64 <= 2^24
        inp = P.attn_grad_inputs(c, "a")
        ref, den = P.attn_grad_reference(c, inp["Y"], inp["gelr"])
        assert (den.max() if c.N else 0) < 2 ** 24 and torch.equal(ref, ref.round()), c.name
    for c in P.HEAD_MEAN_CASES:
        inp = P.head_mean_inputs(c, "a")
        ref, den = P.head_mean_reference(c, inp["X"])
        assert torch.equal(ref, ref.round()), c.name
        assert torch.equal(P.head_mean_emulation(c, inp["X"]).double(), ref), c.name
        g = inp["gR"].double() / c.H
        assert torch.equal(g, g.round()), c.name


# ------------------------------------------------------------------ 2. the 32 instances
def test_proj_labels_cover_every_instance():
    assert len(P.PROJ_INSTANCES) == 32
    cases = P.PROJ_CASES + list(P.PROJ_MAXIMA)
    have = {lab for c in cases for lab in c.labels}
    missing = [lab for lab in P.PROJ_REQUIRED_LABELS if lab not in have]
    assert not missing, missing
    assert have <= set(P.PROJ_REQUIRED_LABELS)
    names = [c.name for c in cases]
    assert len(set(names)) == len(names)
    for algo, tile in P.PROJ_PATHS:
        mine = [c for c in P.PROJ_CASES if (c.algo, c.tile) == (algo, tile)]
        assert set(P.PROJ_ROWS) <= {c.N for c in mine}, (algo, tile)
        assert {4, 16, 74, 75, 76, 80} <= {c.K for c in mine}
        assert any(c.off_x % 4 for c in mine) and any(c.K == 80 and c.ldx == 84 for c in mine)
        assert {4, 24, 48, 96} <= {c.F for c in mine} and {1, 2, 4, 8} <= {c.H for c in mine}
        assert {P.RES_PROJ, P.RES_MEAN, P.RES_NONE} <= {c.res for c in mine}
        assert {(4, 8), (24, 24), (24, 48), (48, 48), (48, 96), (384, 768)} <= {(c.HF, c.C) for c in mine}
    for c in cases:
        assert c.H in (1, 2, 4, 8) and c.F % 4 == 0 and c.N <= 520 and c.C <= 1536 and c.K <= 80, c.name
        if c.wide:   # fast / guarded is exactly x3w_fast of the placed operands
            assert c.fast == (c.ldx % 4 == 0 and c.ldw % 4 == 0 and c.off_x % 4 == 0 and c.K % 4 == 0)
    # more tiles than the persistent cap at gemm_persist = 8, and one workgroup per tile at 0
    for algo in ("bf16", "f16x2", "x3"):
        per = {c.persist for c in P.PROJ_CASES if c.algo == algo and c.wide
               and -(-c.N // 256) * -(-c.C // 256) > 8}
        assert {0, 8} <= per, algo
    assert {c.maxima for c in P.PROJ_MAXIMA} == {"given", "null", "one"}
    assert [P.proj_logw(f) for f in (4, 24, 48, 96, 12, 64)] == [2, 3, 4, 5, 2, 5]


# ------------------------------------------------------------------ 3. fold / unfold adjoint
def test_fold_unfold_adjoint():
    """<fold(fc, res), gW> == <fc, g_fc> + <res, g_res> in float64: the two references agree."""
    for c in P.FOLD_CASES:
        if c.Fin > 100:
            continue
        g = torch.Generator().manual_seed(7)
        fc = torch.randn((c.HF, c.Fin), generator=g, dtype=torch.float64)
        res = torch.randn((c.HF, c.Fin), generator=g, dtype=torch.float64)
        a = torch.randn((2, c.HF), generator=g, dtype=torch.float64)
        gW = torch.randn((c.rows, c.Fin), generator=g, dtype=torch.float64)
        Wcat, _ = P.fold_reference(c, fc, res, a)
        g_fc, g_res, _ = P.unfold_reference(c, gW, a)
        lhs = (Wcat * gW).sum()
        rhs = (fc * g_fc).sum() + ((res * g_res).sum() if g_res is not None else 0.0)
        scale = (Wcat.abs() * gW.abs()).sum()
        assert abs(lhs - rhs) <= 1e-13 * scale, (c.name, float(lhs), float(rhs))


# ------------------------------------------------------------------ 4. the re-association
def test_attn_grad_reassociation():
    """sum_k G[h, k] fc.weight[hF + f, k] with G = gelr^T X equals the attention-vector gradient of
    Y = X fc.weight^T (float64): what GATLayerFunction.backward computes instead of attn_grad."""
    c = P.AttnGrad(257, 4, 24, 0)
    g = torch.Generator().manual_seed(11)
    X = torch.randn((c.N, 75), generator=g, dtype=torch.float64)
    W = torch.randn((c.HF, 75), generator=g, dtype=torch.float64)
    gelr = torch.randn((c.N, 2 * c.H), generator=g, dtype=torch.float64)
    ref, den = P.attn_grad_reference(c, X @ W.t(), gelr)
    G_ = (gelr.t() @ X).reshape(2, c.H, 1, 75)
    re = (G_ * W.reshape(1, c.H, c.F, 75)).sum(-1).reshape(2, c.HF)
    assert ((re - ref).abs() <= 1e-12 * (gelr.abs().t() @ X.abs()).max() * W.abs().sum(1).max()).all()


# ------------------------------------------------------------------ 5. emulations inside the bars
def test_fold_unfold_emulation_inside_bars():
    for c in P.FOLD_CASES:
        inp = P.fold_inputs(c, "b")
        ref, den = P.fold_reference(c, inp["fc"], inp["res"], inp["a"])
        emu = P.fold_emulation(c, inp["fc"], inp["res"], inp["a"]).double()
        assert ((emu - ref).abs() <= P.fold_bar(c)[:, None] * den).all(), c.name
        un = P.unfold_inputs(c, "b")
        g_fc, g_res, den = P.unfold_reference(c, un["gW"], un["a"])
        assert ((P.unfold_emulation(c, un["gW"], un["a"]).double() - g_fc).abs() <= 2 * P.U * den).all(), c.name
        if c.res == P.RES_MEAN:
            got = (un["gW"][c.HF:c.HF + c.F] / float(c.H)).repeat(c.H, 1).double()
            if P.pow2(c.H):
                assert torch.equal(got, g_res), c.name
            else:
                assert ((got - g_res).abs() <= P.U * g_res.abs()).all(), c.name


@pytest.mark.parametrize("c", P.ATTN_GRAD_CASES, ids=lambda c: c.name)
def test_attn_grad_plan_and_emulation(c):
    S, rows_per, depth = P.attn_grad_plan(c.N, c.HF)
    assert depth == c.depth, (c.name, S, rows_per, depth)
    assert S * rows_per >= c.N and (S == 1 or (S - 1) * rows_per < c.N)
    inp = P.attn_grad_inputs(c, "b")
    ref, den = P.attn_grad_reference(c, inp["Y"], inp["gelr"])
    emu = P.attn_grad_emulation(c, inp["Y"], inp["gelr"]).double()
    assert ((emu - ref).abs() <= c.depth * P.U * den).all(), c.name
    ia = P.attn_grad_inputs(c, "a")
    ra, _ = P.attn_grad_reference(c, ia["Y"], ia["gelr"])
    assert torch.equal(P.attn_grad_emulation(c, ia["Y"], ia["gelr"]).double(), ra), c.name


def test_attn_grad_table_reaches_every_edge():
    ns = {c.N for c in P.ATTN_GRAD_CASES}
    assert {0, 1, 3, 4, 5, 255, 256, 257, 1025, 2049} <= ns
    assert {3, 256, 260, 1536} <= {c.HF for c in P.ATTN_GRAD_CASES}
    assert max(P.attn_grad_plan(c.N, c.HF)[0] for c in P.ATTN_GRAD_CASES) >= 8
    assert any(P.attn_grad_plan(c.N, c.HF)[1] % 4 for c in P.ATTN_GRAD_CASES)      # the row tail runs


def test_head_mean_emulation_inside_bar():
    for c in P.HEAD_MEAN_CASES:
        inp = P.head_mean_inputs(c, "b")
        ref, den = P.head_mean_reference(c, inp["X"])
        emu = P.head_mean_emulation(c, inp["X"]).double()
        assert ((emu - ref).abs() <= c.H * P.U * den).all(), c.name
        got = (inp["gR"] / float(c.H)).double()
        want = inp["gR"].double() / c.H
        if P.pow2(c.H):
            assert torch.equal(got, want), c.name
        else:
            assert ((got - want).abs() <= P.U * want.abs()).all(), c.name
    assert {1, 2, 3, 4, 8} <= {c.H for c in P.HEAD_MEAN_CASES}
    assert {0, 1, 63, 65, 257} <= {c.N for c in P.HEAD_MEAN_CASES}
    assert {(1, 24 * 75), (1, 96 * 768)} <= {(c.N, c.F) for c in P.HEAD_MEAN_CASES}


def test_proj_elr_emulation_vs_cpu_bar():
    """The epilogue's summation order (butterfly over W columns, then F / W partials in sequence) on
    an fp32 Y, measured against the bar the GPU test holds elr to: printed, and inside it."""
    worst = 0.0
    for c in P.PROJ_CASES:
        if c.algo != "f32" or c.N > 257:
            continue
        inp = P.proj_inputs(c, "b")
        Y, elr, den_y, den_el = P.proj_reference(c, inp)
        y32, el32 = P.proj_cpu_fp32(c, inp)
        b = G.bar(G.stat(el32, elr, den_el))
        e = G.stat(P.proj_epilogue_emulation(c, y32, inp["a"]), elr, den_el)
        worst = max(worst, e / b)
        assert e <= b, (c.name, e, b)
    print(f"epilogue-order emulation: worst e / bar = {worst:.3f}")
