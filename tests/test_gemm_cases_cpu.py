"""CPU conditions on the GEMM edge cases of _gemm_cases.py (no GPU): what test_gpu_gemm_edges.py
relies on must hold for every case in the tables.

 * kind (a) inputs are exact: the emulated split-fp16 low planes of A (with the entry's own scale:
   per row or operand-wide) and of B are identically zero, every value has at most 4 significant
   bits (split-bf16, plain bf16), and torch's CPU fp32 product reproduces the float64 reference
   cast to fp32 bit for bit — with the result summed forwards, backwards and in two halves;
 * every path label of the tables occurs, and every table keeps its product below the size
   budget;
 * the bar 3 * 2^-22 + 4 e_cpu holds for the split-fp16 product emulated on the CPU, and an
   emulation with the l_a h_b cross term left out exceeds it at least tenfold at every K of the
   tables.
"""
import pytest
import torch

import _gemm_cases as G

GROUPS = G.groups()


@pytest.mark.parametrize("group", sorted(GROUPS))
def test_exact_inputs_are_exact(group):
    for c in GROUPS[group]:
        if "a" not in c.kind_list():
            continue
        inp = G.make_inputs(c, "a")
        A, B = inp["A"], inp["B"]
        # <= 4 significant bits: bf16 (8 bits) holds every value, its second and third terms are zero
        assert torch.equal(A.bfloat16().float(), A) and torch.equal(B.bfloat16().float(), B), c.name
        sa = G.a_shift(c, A)
        sb = G.amax_shift(B.abs().max())
        ha, la = G.split2h(A, sa)
        hb, lb = G.split2h(B, sb)
        assert not la.any() and not lb.any(), c.name
        assert torch.isfinite(ha).all() and torch.isfinite(hb).all(), c.name
        if c.M >= 3:
            assert not A[:, c.M // 2].any(), c.name          # the all-zero row
        ref, pre, _ = G.reference(c, inp)
        ref32 = pre.float()
        assert torch.equal(ref32.double(), pre), c.name       # the float64 result IS an fp32 number
        assert torch.equal(G.cpu_fp32_pre(c, inp), ref32), c.name
        # another summation order gives the same bits: k backwards, and two halves added last
        Af, Bf = A.flip(2), B.flip(2)
        flipped = dict(inp, A=Af, B=Bf)
        assert torch.equal(G.cpu_fp32_pre(c, flipped), ref32), c.name
        h = c.K // 2
        if h:
            halves = A[:, :, :h] @ B[:, :, :h].transpose(1, 2) + A[:, :, h:] @ B[:, :, h:].transpose(1, 2)
            full = G.cpu_fp32_pre(c, dict(inp, bias=None, C0=None))
            assert torch.equal(halves, full), c.name
        if c.act in (0, 1, 3):
            # the activation keeps exactness (ReLU; ELU' factors 0, 1/2, 1)
            assert torch.equal(ref.float().double(), ref), c.name
        if c.entry == "colsum":
            s, _ = G.colsum_reference(c, inp)
            assert torch.equal(s.float().double(), s), c.name
            rows = A[0, c.sum_off:c.sum_off + c.sum_n]
            assert torch.equal(c.alpha * rows.sum(1), s.float()), c.name


def test_exponent_ranges():
    """e spans 0 .. 20 on per-row entries, 0 .. 8 on operand-wide ones, <= 16 with addends; the
    unit-to-top span of every exact result fits 24 bits."""
    for c in G.CASES:
        wide = c.entry in G.OPERAND_WIDE
        add = c.bias or c.beta != 0.0
        assert c.emax <= 8 if wide else (c.emax == 16 if add else c.emax == 20), c.name
        top = max(c.K * 64, 2 ** (c.emax + 5) if add else 0) * 2   # |sum| + addends, in units of 2^-e
        assert top <= 2 ** 24, c.name
        if c.M >= 2 and "a" in c.kind_list():
            A = G.make_inputs(c, "a")["A"]
            mx = A.abs().amax(2)
            assert torch.equal(A[:, 0], A[:, 0].round()), c.name   # e = 0: integers
            assert mx[:, c.M - 1].max() <= 8 * 2.0 ** -c.emax, c.name


def test_labels_and_budget():
    have = {lab for c in G.CASES for lab in c.labels}
    missing = [lab for lab in G.REQUIRED_LABELS if lab not in have]
    assert not missing, missing
    assert all(c.labels for c in G.CASES)
    names = [c.name for c in G.CASES]
    assert len(set(names)) == len(names)
    for c in G.CASES:
        assert c.M <= 800 and c.N <= 800 and c.batch * c.M * c.N * c.K <= 800 * 800 * 2100, c.name
        if c.K > 2100:
            assert c.M * c.N <= 130 * 130, c.name
        if c.entry == "f16x2_rows" or c.entry == "f16x2_ex":
            assert c.ak == 0, c.name
        if c.il4 or c.entry == "f16x2_bsplit":
            assert G.image_ok(c) and c.pad_b % 4 == 0, c.name
        if c.entry == "f16x2_ex":
            assert G.x3w_fast(c), c.name              # the entry's own precondition
        if c.smallk == 1:
            assert c.K <= G.SK_MAX_K and c.K % 4 == 0 and c.N % 4 == 0 and c.ldc % 4 == 0 and c.beta == 0
    # the tables of the issue, dimension by dimension
    t256 = [c for c in G.CASES if c.group == "tile256" and c.entry == "f16x2_amax" and (c.ak, c.bk) == (0, 0)]
    assert {1, 31, 33, 128, 129, 255, 256, 257} <= {c.M for c in t256}
    assert {1, 4, 63, 65, 252, 256, 257, 260} <= {c.N for c in t256}
    assert {4, 12, 16, 20, 36, 76, 1, 17, 74} <= {c.K for c in t256}
    for k in (4, 12, 16, 20, 36, 76):
        assert any("tile256-fast" in c.labels for c in t256 if c.K == k)
    for k in (1, 17, 74):
        assert all("tile256-guarded" in c.labels for c in t256 if c.K == k)
    t128 = [c for c in G.CASES if c.group == "tile128" and c.entry == "f32"]
    assert {1, 63, 65, 127, 128, 129} <= {c.M for c in t128} & {c.N for c in t128}
    assert {4, 31, 32, 33, 36, 74} <= {c.K for c in t128}
    sk = [c for c in G.CASES if c.group == "smallk" and c.smallk == 1]
    assert {4, 16, 20, 32, 48, 52, 64, 76, 80, 96} <= {c.K for c in sk}
    assert {1, 15, 16, 17, 70} <= {c.M for c in sk} and {4, 60, 64, 68, 132} <= {c.N for c in sk}
    assert {G.ks16_plan(c.K) for c in sk} == {1, 2, 3, 4, 5, 6}


def _emulation_case(K, seed):
    g = torch.Generator().manual_seed(seed)
    A = torch.randn((1, 96, K), generator=g) * torch.pow(2.0, -torch.randint(0, 21, (1, 96, 1), generator=g).float())
    B = torch.randn((1, 80, K), generator=g)
    return A, B


@pytest.mark.parametrize("K", G.all_ks())
def test_bar_on_emulated_split(K):
    """The emulated three-product split-fp16 GEMM (per-row A scales) sits under the bar; without
    l_a h_b it is at least ten bars out."""
    A, B = _emulation_case(K, 1000 + K)
    ref = A.double() @ B.double().transpose(1, 2)
    den = A.double().abs() @ B.double().abs().transpose(1, 2)
    e_cpu = G.stat(A @ B.transpose(1, 2), ref, den)
    sa = G.amax_shift(A.abs().amax(2, keepdim=True))
    sb = G.amax_shift(B.abs().max())
    e = G.stat(G.emulate_split(A, B, sa, sb), ref, den)
    e_drop = G.stat(G.emulate_split(A, B, sa, sb, drop=True), ref, den)
    b = G.bar(e_cpu)
    print(f"K={K} e={e:.3e} e_cpu={e_cpu:.3e} bar={b:.3e} dropped={e_drop:.3e}")
    assert e <= b, (e, b)
    assert e_drop >= 10 * b, (e_drop, b)


def test_stat_and_first_diff():
    ref = torch.tensor([[1.0, 2.0], [0.0, 4.0]], dtype=torch.float64)
    den = torch.tensor([[1.0, 2.0], [0.0, 8.0]], dtype=torch.float64)
    x = ref.float().clone()
    assert G.stat(x, ref, den) == 0.0
    x[1, 1] = 5.0
    assert G.stat(x, ref, den) == 0.125
    x[1, 0] = 1e-30                          # den == 0: anything but the reference is infinite
    assert G.stat(x, ref, den) == float("inf")
    n, idx = G.first_diff(x, ref.float())
    assert (n, idx) == (2, (1, 0))
    assert G.bar(0.0) == 3 * 2.0 ** -22
