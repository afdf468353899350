"""CPU conditions on _schnet_cases.py (no GPU): what test_gpu_schnet_kernels.py relies on.

 a. the tables reach every axis value, instance edge, dW_1 split regime and list length named there;
 b. the float64 restatements agree with _schnet_ref and with autograd;
 c. the reference alone stays inside every bar (the float32 CPU run, and the CPU emulation of the
    split path), no den is 0 where the reference is not, no reference quantity is all zero;
 d. the special regimes are what they claim (onehot, exact2, the exact aggregation inputs, zero rows);
 e. the bars catch the mutations of the split path, the lists and ssp;
 f. every refusal breaks exactly one documented condition and is refused without a GPU.

One mutation the bars cannot catch, and why: ONE scale for all of s1 in the FORWARD.  fp16 is a
floating format, so a row 2^-r below the largest loses nothing of its high plane down to r = 29 and
of its low plane down to r = 17; below that the low plane's step is 2^-24 / scale = max|s1| 2^-39.
s1 <= sum |W_1| + |b_1| is of order 10 on any input W_1's own operand-wide scale still represents, so
the loss is below 1e-10 absolute, while ssp itself (log1p(exp x) - ln 2, a cancellation at ln 2)
is only good to u ln 2 = 4e-8 absolute: no sound bar separates the two.  What the per-row scale
gives the forward is that a slot's bits do not depend on its batch, which the emulation shows here
and the GPU file holds bitwise.  In the BACKWARD the rows of dpre2 = dA[dst] hv[src] ssp' do sit 2^-40
apart in the `rows` regime and den is row-relative: there the mutation must exceed the bar."""
import ctypes

import pytest
import torch

import _schnet_cases as S
import _schnet_ref as SR
from mvml_gat import _lib

F64, F32 = torch.float64, torch.float32


# ------------------------------------------------------------------ a. what the tables reach
def test_filter_table():
    C = S.F_CASES
    assert {c.E for c in C} == set(S.F_E) and {c.H for c in C} == set(S.F_H) and {c.K for c in C} == set(S.F_K)
    assert {c.ldd for c in C} == {1, 3} and len({c.name for c in C}) == len(C)
    for ntb, (first, last) in {2: (16, 32), 4: (48, 64), 8: (80, 128)}.items():
        assert S.instance(first) == S.instance(last) == ntb and (last == S.MAX_H or S.instance(last + 16) != ntb)
        assert first == 16 or S.instance(first - 16) != ntb
        assert {c.E for c in C if c.ntb == ntb} >= set(S.F_EDGES), ntb
        assert {c.H for c in C if c.ntb == ntb} >= {first, last}
    for i in range(6):
        assert {c.pads[i] for c in C} == set(S.PADS), i
    assert all(len(set(c.pads)) > 1 for c in C)
    for regime in S.REGIMES[1:]:
        sub = S.regime_cases(regime)
        assert {c.ntb for c in sub} == {2, 4, 8} and any(c.E % S.TILE for c in sub) and len(sub) >= 6, regime
    one = S.regime_cases("onehot")
    assert {32, 80, 112} <= {c.H for c in one} and max(c.K for c in one) == 300
    assert any(c.E == 1 for c in S.regime_cases("rows")) and any(c.E > S.TILE for c in S.regime_cases("rows"))


def test_dw1_table():
    C = S.D_CASES
    assert {c.E for c in C} == set(S.F_E) | set(S.D_BIG) and {c.K for c in C} >= set(S.D_K)
    assert {(c.E, c.K) for c in C if c.E in S.D_BIG} == {(e, k) for e in S.D_BIG for k in (1, 65)}
    assert all(c.H == 16 for c in C if c.E in S.D_BIG)
    assert {c.accumulate for c in C} == {0, 1} == {c.accumulate for c in C if c.E in S.D_BIG}
    # dw1_splits / per, restated from the source
    assert [S.dw1_splits(e) for e in (1, 128, 129, 256, 257, 16256, 16257, 16384, 16385, 10 ** 6)] == \
        [1, 1, 2, 2, 3, 127, 128, 128, 128, 128]
    assert [S.dw1_per(e) for e in (1, 128, 129, 385, 16384, 16385, 16417)] == [32, 128, 96, 128, 128, 160, 160]
    sp = {c.E: S.dw1_splits(c.E) for c in C}
    assert {1, 2, 128} <= set(sp.values())
    assert S.dw1_empty_ranges(16384) == 0 and sp[16384] == 128                  # 128, uncapped
    assert S.dw1_empty_ranges(16385) == 25 and S.dw1_empty_ranges(16417) == 25  # capped: trailing empty ranges
    for c in C:
        S_, per = S.dw1_splits(c.E), S.dw1_per(c.E)
        assert S_ * per >= c.E and per % S.WG_E == 0, c.name
        assert c.E <= 16384 or -(-c.E // (4 * S.WG_E)) > S.MAX_SPLITS
    assert {(c.K + 63) // 64 for c in C} >= {1, 2, 8}                           # blockIdx.y
    assert any(c.E % S.WG_E == 1 for c in C) and any(c.E % S.WG_E == 0 for c in C)
    assert len({c.name for c in C}) == len(C)


def test_aggregation_table():
    C = S.A_CASES
    assert {c.N for c in C} == set(S.A_N) and {c.H for c in C} == set(S.A_H) and {c.direction for c in C} == set(S.A_DIRS)
    seen = set()
    for c in C:
        dg = c.degrees
        assert len(dg) == c.N and set(dg) <= set(S.A_DEGS), c.name
        seen |= set(dg)
        if c.N >= 2:
            assert (dg[0], dg[1]) == (129, 0)
        inp = S.agg_inputs(c)
        x = inp["xidx"].tolist()
        assert max(x) == c.N + 1 and len(set(x)) < len(x) or inp["E"] < 2, c.name
        assert inp["rowptr"].dtype == inp["xidx"].dtype == torch.int32 and int(inp["rowptr"][-1]) == inp["E"]
        if c.direction == "out":
            assert sorted(inp["widx"].tolist()) == list(range(inp["E"])) and inp["widx"].tolist() != list(range(inp["E"]))
        else:
            assert inp["widx"] is None
    assert seen == set(S.A_DEGS)
    for lw in (16, 64):                                     # both instances, both directions, the hub beside the empty list
        for dr in S.A_DIRS:
            assert any(S.agg_instance(c.H) == lw and c.direction == dr and c.N >= 2 for c in C)
    assert {c.H for c in C if c.N == 1} >= {16, 128} and {c.degrees[0] for c in C if c.N == 1} == {17, 65, 129}
    assert len({c.name for c in C}) == len(C)


def test_ssp_table():
    assert {c.n for c in S.S_CASES} == set(S.S_N) and S.S_N[-1] == S.SSP_GRID_CAP + 1
    assert sum(c.n > S.SSP_GRID_CAP for c in S.S_CASES) == 1
    assert {c.inplace for c in S.S_CASES} == {False, True}
    want = torch.tensor(S.S_PLANTED, dtype=F32)
    assert {0.0, 2.0 ** -30, -2.0 ** -30, 1.0, -1.0, 20.0, 88.0, -20.0, -104.0} <= set(want.tolist())
    for c in S.S_CASES:
        inp = S.ssp_inputs(c)
        if c.n > 1:
            assert set(want.tolist()) <= set(inp["x"].tolist()), c.name
            assert torch.equal(inp["x"][c.n - len(want):], want)
        assert torch.isfinite(inp["x"]).all() and torch.isfinite(inp["y"]).all()


# ------------------------------------------------------------------ b. independent references
def _close(a, b, what, den=None):
    den = b.abs().max().clamp_min(1e-300) if den is None else den
    assert bool(((a - b).abs() <= 1e-12 * den).all()), what


@pytest.mark.parametrize("c", S.F_CASES[::5], ids=lambda c: c.name)
def test_filter_reference_vs_autograd(c):
    inp = S.filter_inputs(c, "normal")
    r = S.filter_fwd(inp)
    W1, W2 = inp["W1"].double().requires_grad_(), inp["W2"].double()
    he = SR.filter(inp["d"].double(), inp["centers"].double(), inp["gamma"], W1, inp["b1"].double(), W2, inp["b2"].double())
    _close(r["he"], he.detach(), c.name)
    # the backward from the exact s1 / he, against autograd through a = cfconv(hv, he)
    hv = inp["hv"].double()
    a = SR.cfconv(inp["src"].long(), inp["dst"].long(), S.NODES, hv, he)
    a.backward(inp["dA"].double())
    dp2, dp1 = S.filter_bwd(inp, r["s1"], r["he"])
    dW1 = dp1.T @ r["rbf"]
    _close(dW1, W1.grad, c.name, den=dp1.abs().T @ r["rbf"] + 1e-300)
    # ssp' from the output is ssp' from the input
    _close(S.sspg(r["he"]), torch.sigmoid(r["pre2"]), c.name, den=torch.ones(()))


def test_aggregation_reference_vs_cfconv():
    for c in S.A_CASES[::3]:
        inp = S.agg_inputs(c)
        w = torch.arange(inp["E"]) if inp["widx"] is None else inp["widx"].long()
        # _schnet_ref.cfconv with the list's (source row, owner, weight row) as its (src, dst, he)
        want = SR.cfconv(inp["xidx"].long()[w], inp["owner"], c.N, inp["X"].double(), inp["Wt"].double()[w])
        loop = torch.zeros((c.N, c.H), dtype=F64)
        for v in range(c.N):
            for i in range(int(inp["rowptr"][v]), int(inp["rowptr"][v + 1])):
                wi = i if inp["widx"] is None else int(inp["widx"][i])
                loop[v] += inp["X"][int(inp["xidx"][wi])].double() * inp["Wt"][wi].double()
        _close(S.agg_eval(c, inp), loop, c.name, den=S.agg_eval(c, inp, absolute=True) + 1e-300)
        _close(want, loop, c.name, den=S.agg_eval(c, inp, absolute=True) + 1e-300)


# ------------------------------------------------------------------ c. the reference alone is inside the bars
def _hold32(name, r32, ref, den, limit=0.25):
    assert torch.isfinite(ref).all() and torch.isfinite(den).all() and torch.isfinite(r32).all(), name
    assert not bool(((den == 0) & (ref != 0)).any()), name
    rec, ok = S.fp32_check(r32, ref, den, r32)
    assert ok and rec["ratio"] <= limit + 1e-12 and rec["bar_floor"] < 2e-5, (name, rec)
    return rec


def _inside(name, got, ref, allowed, limit):
    assert not bool(((allowed == 0) & (ref != 0)).any()), name
    rec, ok = S.allowed_check(got, ref, allowed)
    assert ok and rec["ratio"] <= limit, (name, rec)
    return rec["ratio"]


@pytest.mark.parametrize("regime", S.REGIMES)
def test_filter_references_inside_their_bars(regime):
    """The float32 CPU run within 1/4 of every bar by construction, the CPU emulation of the split
    path within the bar."""
    worst = 0.0
    for c in S.regime_cases(regime):
        inp = S.filter_inputs(c, regime)
        r, a, al, pcs = S.fwd_bars(inp)
        r32 = S.filter_fwd(inp, F32)
        assert all(v < 2e-5 for v in pcs.values()), (c.name, pcs)
        for k in ("s1", "he"):
            assert bool(r[k].abs().max() > 0) and torch.isfinite(r[k]).all(), (c.name, k)
            _inside(c.name + k + " r32", r32[k], r[k], al[k], 0.25 if k == "s1" else 0.5)
        es1, ehe = S.emulate_fwd(inp)
        worst = max(worst, _inside(c.name + "s1 emu", es1, r["s1"], al["s1"], 1.0), _inside(c.name + "he emu", ehe, r["he"], al["he"], 1.0))
        s1, he = S.bwd_given(inp)
        rb, ab, r32_2, alb, pb = S.bwd_bars(inp, s1, he)
        assert all(v < 2e-5 for v in pb.values()), (c.name, pb)
        _hold32(c.name + "dpre2", r32_2, rb[0], ab[0])
        _inside(c.name + "dpre1 r32", S.filter_bwd(inp, s1, he, F32)[1], rb[1], alb, 0.5)
        worst = max(worst, _inside(c.name + "dpre1 emu", S.emulate_bwd(inp, s1, he)[1], rb[1], alb, 1.0))
        only_zero_row = c.E == 1 and regime == "rows"        # (its one slot is the documented zero row)
        assert bool(rb[1].abs().max() > 0) or regime == "zero_w2" or only_zero_row, c.name
        assert bool(rb[0].abs().max() > 0) or only_zero_row, c.name
    print(f"{regime}: the emulated split path reaches {worst:.3f} of its bars")


def test_other_references_inside_their_bars():
    for c in S.D_CASES:
        inp = S.dw1_inputs(c)
        ref = S.dw1_eval(c, inp)
        assert bool(ref.abs().max() > 0)
        _hold32(c.name, S.dw1_eval(c, inp, F32), ref, S.dw1_eval(c, inp, absolute=True))
    for c in S.A_CASES:
        inp = S.agg_inputs(c)
        ref = S.agg_eval(c, inp)
        assert bool(ref.abs().max() > 0)
        _hold32(c.name, S.agg_eval(c, inp, F32), ref, S.agg_eval(c, inp, absolute=True))
        empty = [v for v, n in enumerate(c.degrees) if n == 0]
        assert not ref[empty].any() and not S.agg_eval(c, inp, absolute=True)[empty].any()
    for c in S.S_CASES[:-1]:
        inp = S.ssp_inputs(c)
        _hold32(c.name + "fwd", S.ssp_fwd(inp, F32), S.ssp_fwd(inp), S.ssp_fwd(inp, absolute=True))
        _hold32(c.name + "bwd", S.ssp_bwd(inp, F32), S.ssp_bwd(inp), S.ssp_bwd(inp, absolute=True))


# ------------------------------------------------------------------ d. the special regimes
def test_onehot_is_exact():
    for c in S.regime_cases("onehot"):
        inp = S.filter_inputs(c, "onehot")
        assert 0.0 < inp["gamma"] <= 3.0e38 and float(torch.tensor(inp["gamma"], dtype=F32)) == inp["gamma"]  # gamma_ok
        assert torch.equal(inp["centers"], torch.arange(c.K, dtype=F32) * 0.5)
        rbf = S.rbf_of(inp, F32)
        k = torch.arange(c.E) % c.K
        assert set(k.tolist()) == set(range(c.K)), c.name                        # every k < K is hit
        on = torch.zeros_like(rbf, dtype=torch.bool)
        on[torch.arange(c.E), k] = True
        assert bool((rbf[on] == 1.0).all()) and bool((rbf[~on] == 0.0).all()), c.name
        gap2 = float((inp["centers"][1] - inp["centers"][0]) ** 2) if c.K > 1 else 0.25
        assert inp["gamma"] * gap2 >= 110 and float(torch.exp(torch.tensor(-110.0, dtype=F32))) == 0.0
        pre1 = inp["W1"].T[k] + inp["b1"]                                          # one fp32 add: exact?
        assert torch.equal(pre1.double(), inp["W1"].double().T[k] + inp["b1"].double()), c.name
        assert (S.filter_fwd(inp)["pre1"] - pre1.double()).abs().max() < 1e-40
        assert torch.equal(pre1 * 8, (pre1 * 8).round()) and float(pre1.abs().max()) <= 2.0
        assert torch.equal(S.emulate_fwd(inp)[0], SR.ssp(pre1)), c.name          # any correct split path: exact pre1


def test_exact2_is_exact():
    # ssp'(30) from the output is 1 for any expf within a factor of two of exp(-30)
    for f in (0.5, 1.0, 2.0):
        e = torch.tensor(f * 9.357622968840175e-14, dtype=F32)
        assert float(torch.tensor(1.0, dtype=F32) - torch.tensor(0.5, dtype=F32) * e) == 1.0
    assert float(S.sspg(torch.tensor(S.EXACT_Y, dtype=F32))) == 1.0
    for c in S.regime_cases("rows"):
        inp, s1, he = S.exact2_inputs(c)
        dp2, dp1 = S.exact2_expected(inp)
        g, h = inp["dA"].double()[inp["dst"].long()], inp["hv"].double()[inp["src"].long()]
        unit = (g.abs().amax(1, keepdim=True) * h.abs().amax(1, keepdim=True)).clamp_min(2.0 ** -60)
        unit = torch.pow(2.0, torch.floor(torch.log2(unit)) - 6)               # <= the row's integer unit
        assert torch.equal(dp2.double(), g * h)
        assert bool((((g * h).abs() @ inp["W2"].double().abs()) / unit * 8 < 2 ** 24).all()), c.name
        assert torch.equal(dp1.double(), (g * h) @ inp["W2"].double()), c.name
        e2, e1 = S.emulate_bwd(inp, s1, he)
        assert torch.equal(e2, dp2) and torch.equal(e1, dp1), c.name             # the split path is exact on them
        assert not dp2[inp["dst"] == S.ZERO_ROW].any() and not dp1[inp["dst"] == S.ZERO_ROW].any()
        assert bool(dp1.abs().max() > 0) or c.E == 1


def test_exact_aggregation_inputs():
    for c in S.A_CASES:
        inp = S.agg_inputs(c, exact=True)
        ref, den = S.agg_eval(c, inp), S.agg_eval(c, inp, absolute=True)
        unit = torch.pow(2.0, -(torch.arange(c.N) % 21).double())[:, None]
        assert bool((den / unit < 2 ** 24).all()) and torch.equal(den / unit, (den / unit).round()), c.name
        assert torch.equal(ref.float().double(), ref) and torch.equal(S.agg_eval(c, inp, F32).double(), ref), c.name


def test_rows_and_zero_w_regimes():
    for c in S.regime_cases("rows"):
        inp = S.filter_inputs(c, "rows")
        for k in ("hv", "dA"):
            m = inp[k].abs().amax(1)
            assert float(m[m > 0].max() / m[m > 0].min()) > 2.0 ** 17, c.name
        assert not inp["dA"][S.ZERO_ROW].any() and int(inp["dst"][-1]) == S.ZERO_ROW
        s1, he = S.bwd_given(inp)
        dp2, dp1 = S.filter_bwd(inp, s1, he)
        z = inp["dst"] == S.ZERO_ROW
        assert not dp2[z].any() and not dp1[z].any()
        e2, e1 = S.emulate_bwd(inp, s1, he)
        assert not e2[z].any() and not e1[z].any()
        if c.E > 3:
            m = dp2.abs().amax(1)
            assert float(m[~z].max() / m[~z].min()) > 2.0 ** 20, c.name
    for regime, k, b in (("zero_w1", "s1", "b1"), ("zero_w2", "he", "b2")):
        for c in S.regime_cases(regime):
            inp = S.filter_inputs(c, regime)
            rows = inp[b].expand(c.E, c.H).contiguous()      # (the same shape: the same vector path of the CPU's libm)
            assert torch.equal(S.filter_fwd(inp)[k], SR.ssp(rows.double())), c.name
            got = S.emulate_fwd(inp)[0 if k == "s1" else 1]
            assert torch.equal(got, SR.ssp(rows)), c.name
    for c in S.regime_cases("saturated"):
        inp = S.filter_inputs(c, "saturated")
        r = S.filter_fwd(inp)
        for p in ("pre1", "pre2"):
            assert float(r[p].max()) > 20 and float(r[p].min()) < -20, c.name
            g = torch.sigmoid(r[p])
            assert float(g.min()) < 1e-8 and float(g.max()) > 1 - 1e-8


# ------------------------------------------------------------------ e. the mutations the bars must catch
def _ratio(got, ref, allowed):
    return S.allowed_check(got, ref, allowed)[0]["ratio"]


def test_dropped_split_term_exceeds_the_bars():
    low2, lowb = float("inf"), float("inf")
    for c in S.F_CASES:
        inp = S.filter_inputs(c, "normal")
        r, _, al, _ = S.fwd_bars(inp)
        low2 = min(low2, _ratio(S.emulate_fwd(inp, drop2=True)[1], r["he"], al["he"]))
        s1, he = S.bwd_given(inp)
        rb, _, _, alb, _ = S.bwd_bars(inp, s1, he)
        lowb = min(lowb, _ratio(S.emulate_bwd(inp, s1, he, drop=True)[1], rb[1], alb))
    assert low2 > 1 and lowb > 1, f"a dropped l_a h_b term reaches only {low2:.2f} (product 2) / {lowb:.2f} (backward) of the bar"
    print(f"dropped term: at least {low2:.1f} x (product 2), {lowb:.1f} x (backward) the bar")


def test_one_scale_for_all_rows_exceeds_the_backward_bar():
    low = float("inf")
    for c in S.regime_cases("rows"):
        if c.E <= 3:
            continue
        inp = S.filter_inputs(c, "rows")
        s1, he = S.bwd_given(inp)
        rb, _, _, alb, _ = S.bwd_bars(inp, s1, he)
        low = min(low, _ratio(S.emulate_bwd(inp, s1, he, global_scale=True)[1], rb[1], alb))
    assert low > 1, f"one scale for every dpre2 row reaches only {low:.2f} of the bar"
    print(f"one scale for dpre2: at least {low:.1f} x the bar")


def test_one_scale_for_s1_changes_the_bits_with_the_batch():
    """The module docstring: below any sound bar in the forward, so what is shown is what the GPU file
    holds bitwise -- a slot's bits with a per-row scale do not depend on the batch, with one scale
    they do."""
    c = next(c for c in S.F_CASES if (c.H, c.E) == (64, 385))
    inp = S.filter_inputs(c, "normal")
    r, _, al, _ = S.fwd_bars(inp)
    assert _ratio(S.emulate_fwd(inp, global_scale=True)[1], r["he"], al["he"]) < 1
    # (a scale moves no bit of an fp16 plane until the low plane goes subnormal, 2^17 below the largest row)
    inp["W1"][:, 0] *= 4.0e6                                 # slot 0 (d = 0, on centre 0) is the batch's largest row
    small = S.emulate_fwd(inp)[0].abs().amax(1) < 16.0       # the slots that centre 0 does not reach
    assert 100 < int(small.sum()) < c.E
    sub = dict(inp, d=inp["d"][small])
    for gs, same in ((False, True), (True, False)):
        full, part = S.emulate_fwd(inp, global_scale=gs)[1], S.emulate_fwd(sub, global_scale=gs)[1]
        assert torch.equal(full[small], part) == same, gs


def test_swapped_w1_columns_exceed_the_onehot_bar():
    low = float("inf")
    for c in S.regime_cases("onehot"):
        if c.K < 2:
            continue
        inp = S.filter_inputs(c, "onehot")
        k = next(k for k in range(c.K - 1) if k // 16 == (k + 1) // 16 and not torch.equal(inp["W1"][:, k], inp["W1"][:, k + 1]))
        pre1 = S.filter_fwd(inp)["pre1"]
        ref, den = SR.ssp(pre1), S._sp(pre1.abs())
        got = S.emulate_fwd(inp, swap_w1=(k, k + 1))[0]
        rec, ok = S.fp32_check(got, ref, den, SR.ssp(pre1.float()))
        assert S.fp32_check(S.emulate_fwd(inp)[0], ref, den, SR.ssp(pre1.float()))[1]
        low = min(low, rec["ratio"])
        assert not ok
    assert low > 1, f"two swapped W_1 columns reach only {low:.2f} of the ssp bar"
    print(f"swapped W_1 columns: at least {low:.0f} x the bar")


def test_left_out_last_slot_or_entry_exceeds_the_bars():
    low = float("inf")
    for c in S.F_CASES:                                      # the last slot of a tile never computed: zeros
        if c.E % S.TILE == 0:
            continue
        inp = S.filter_inputs(c, "normal")
        r, _, al, _ = S.fwd_bars(inp)
        for k, got in zip(("s1", "he"), S.emulate_fwd(inp)):
            got = got.clone()
            got[-1] = 0.0
            low = min(low, _ratio(got, r[k], al[k]))
    for c in S.D_CASES:
        inp = S.dw1_inputs(c)
        ref, den = S.dw1_eval(c, inp), S.dw1_eval(c, inp, absolute=True)
        rec, ok = S.fp32_check(S.dw1_eval(c, inp, F32, leave_out_last=True), ref, den, S.dw1_eval(c, inp, F32))
        low = min(low, rec["ratio"])
        assert not ok, c.name
    for c in S.A_CASES:
        if not {17, 65} & set(c.degrees):
            continue
        inp = S.agg_inputs(c)
        ref, den = S.agg_eval(c, inp), S.agg_eval(c, inp, absolute=True)
        rec, ok = S.fp32_check(S.agg_eval(c, inp, F32, leave_out_last_of=(17, 65)), ref, den, S.agg_eval(c, inp, F32))
        low = min(low, rec["ratio"])
        assert not ok, c.name
    assert low > 1, f"a left-out last slot or list entry reaches only {low:.2f} of its bar"
    print(f"left-out slot / entry: at least {low:.0f} x the bar")


def test_ssp_without_the_threshold_branch_fails_at_89():
    """fp32 exp(88) = 1.65e38 is still finite, so log1p(exp(88)) is right; at 89 it is inf."""
    assert torch.isfinite(torch.exp(torch.tensor(88.0, dtype=F32))) and torch.isinf(torch.exp(torch.tensor(89.0, dtype=F32)))
    c = S.SC(257, False)
    inp = S.ssp_inputs(c)
    bad = S.ssp_fwd(inp, F32, threshold=False)
    assert bool(torch.isinf(bad[inp["x"] == 89.0]).all())
    rec, ok = S.fp32_check(bad, S.ssp_fwd(inp), S.ssp_fwd(inp, absolute=True), S.ssp_fwd(inp, F32))
    assert not ok and rec["ratio"] == float("inf")


# ------------------------------------------------------------------ f. the refusals, without a GPU
REFUSALS = S.refusals(ctypes.c_void_p(4096), ctypes.c_void_p(4100))


def test_refusal_table_breaks_one_condition_each():
    for entry in S.SPEC:
        assert S.violations(entry, S._good(entry, ctypes.c_void_p(4096))) == [], entry
    for what, (entry, who, code, args) in REFUSALS.items():
        v = S.violations(entry, args)
        assert len(v) == 1, (what, v)
        assert (code == S.WORKSPACE) == v[0].startswith("workspace"), what
    protos = _lib.parse_header()
    for entry, sp in S.SPEC.items():
        assert len(protos[entry][1]) == len(sp["args"].split()), entry
        n_ptr = sum(1 for a in protos[entry][1] if a is ctypes.c_void_p) - 1   # all but the stream
        optional = 1 if entry == "mvml_cfconv_agg" else 0                      # widx
        nulls = sum(1 for k in REFUSALS if k.startswith(entry + ":") and k.endswith(" NULL"))
        assert nulls == n_ptr - optional, entry
    L = _lib.lib()
    assert L.mvml_schnet_dw1_workspace_size(S.RE, S.RH, S.RK) == S.dw1_workspace(S.RE, S.RH, S.RK)
    for c in S.D_CASES:
        assert L.mvml_schnet_dw1_workspace_size(c.E, c.H, c.K) == S.dw1_workspace(c.E, c.H, c.K), c.name
    for c in S.F_CASES:
        assert L.mvml_schnet_image_bytes(c.H, c.K) == S.image_bytes(c.H, c.K), c.name


@pytest.mark.parametrize("what", list(REFUSALS))
def test_refusals_without_gpu(what):
    entry, who, code, args = REFUSALS[what]
    L = _lib.lib()
    rc = getattr(L, entry)(*args)
    msg = L.mvml_last_error().decode(errors="replace")
    assert rc == code, (rc, msg)
    assert who in msg, msg
