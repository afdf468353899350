"""Conditions on the INPUTS of test_gpu_batching_tiers.py, so that no GPU test there can pass for
lack of a hard case: every size class a case names gets a molecule, every class limit has a
molecule exactly at it and one above it, the repeated-key cases repeat keys inside and across
placement chunks (and a non-stable placement of them is a different answer), the persistent
kernels get more list entries than their grids, and the node-group plans straddle every cap.
No GPU: sensitivity of the GPU comparisons is argued here, not by running a wrong kernel."""
import numpy as np
import pytest

import _batching_cases as C
from oracle import graph_ref

K = C.tier_constants()
BIGWAVE_GRID, CSR_GRID = 2048, 512  # the persistent grids' caps in mvml_build_csr's launches


def test_tier_constants():
    assert set(K) == set(C.CONSTANT_NAMES)
    assert all(type(v) is int and v > 0 for v in K.values())
    assert K["kWaveMolAtoms"] < K["kBigMolAtoms"] < K["kLdsNodes"]
    assert K["kWaveMolEdges"] < K["kBigMolEdges"]
    assert K["kPlanWinAtoms"] < K["kPlanBigAtoms"] and K["kPlanEdgeCap"] < K["kPlanBigEdgeCap"]


def test_tier_of_boundary_pairs():
    wa, we, ba, be, la = (K[k] for k in ("kWaveMolAtoms", "kWaveMolEdges", "kBigMolAtoms",
                                         "kBigMolEdges", "kLdsNodes"))
    table = [((wa, we), "W"), ((wa + 1, we), "B"), ((wa, we + 1), "B"), ((ba, be), "B"),
             ((ba + 1, be), "L"), ((ba, be + 1), "L"), ((la, 10 * be), "L"), ((la + 1, 0), "S")]
    assert [C.tier_of(*p) for p, _ in table] == [t for _, t in table]
    assert C.tier_of(0, 0) == "W" and C.tier_of(1, we + 1) == "B" and C.tier_of(wa + 1, 0) == "B"


@pytest.mark.parametrize("name", C.CASE_NAMES)
def test_named_classes_are_present(name):
    c = C.case(name)
    assert set(c.tiers()) == set(c.names), name


def _has(c, pred):
    return any(pred(int(n), int(e)) for n, e in zip(c.bnn, c.bne))


LIMIT_PREDICATES = {  # limit: (a molecule exactly at it, one exactly one above it)
    "W atoms": (lambda n, e: n == K["kWaveMolAtoms"] and e <= K["kWaveMolEdges"],
                lambda n, e: n == K["kWaveMolAtoms"] + 1 and e <= K["kWaveMolEdges"]),
    "W edges": (lambda n, e: n <= K["kWaveMolAtoms"] and e == K["kWaveMolEdges"],
                lambda n, e: n <= K["kWaveMolAtoms"] and e == K["kWaveMolEdges"] + 1),
    "B atoms": (lambda n, e: n == K["kBigMolAtoms"] and e <= K["kBigMolEdges"],
                lambda n, e: n == K["kBigMolAtoms"] + 1 and e <= K["kBigMolEdges"]),
    "B edges": (lambda n, e: n <= K["kBigMolAtoms"] and e == K["kBigMolEdges"],
                lambda n, e: n <= K["kBigMolAtoms"] and e == K["kBigMolEdges"] + 1),
    "L atoms": (lambda n, e: n == K["kLdsNodes"], lambda n, e: n == K["kLdsNodes"] + 1),
}


@pytest.mark.parametrize("name", C.BOUNDARY_CASES)
def test_boundary_cases_straddle_their_limits(name):
    c = C.case(name)
    if name == "w_full":  # whole workgroups of molecules exactly at both class-W limits
        assert len(c.bnn) % 4 == 0 and len(c.bnn) >= 8
        assert np.all(c.bnn == K["kWaveMolAtoms"]) and np.all(c.bne == K["kWaveMolEdges"])
        return
    assert c.limits
    for lim in c.limits:
        at, above = LIMIT_PREDICATES[lim]
        assert _has(c, at), (name, lim, "no molecule at the limit")
        assert _has(c, above), (name, lim, "no molecule one above the limit")


def test_every_limit_is_straddled_somewhere():
    seen = {lim for name in C.BOUNDARY_CASES for lim in C.case(name).limits}
    assert seen == set(LIMIT_PREDICATES)
    assert set(C.case("all_classes").limits) == set(LIMIT_PREDICATES)


def test_w_limits_neighbours_share_a_workgroup():
    """build_csr_wave_kernel takes four consecutive molecules per workgroup: an at-limit
    molecule sits beside a 0-atom and a 1-atom one, and beside another at-limit one."""
    c = C.case("w_limits")
    at = (c.bnn == K["kWaveMolAtoms"]) & (c.bne == K["kWaveMolEdges"])
    groups = [slice(i, i + 4) for i in range(0, len(c.bnn), 4)]
    assert any(at[g].any() and (c.bnn[g] == 0).any() and (c.bnn[g] == 1).any() for g in groups)
    assert any(at[g].sum() >= 2 for g in groups)


@pytest.mark.parametrize("name", C.REPEAT_CASES)
def test_repeat_cases_repeat_keys(name):
    tier = name[-1]
    c = C.case(name)
    chunk = C.chunk_of(tier)
    (hn, he, hk), _ = C.REPEAT_SHAPES[tier]
    assert hk > chunk and c.molecule(c.subjects[0])[0] == hn
    for i in c.subjects:
        n, s, d = c.molecule(i)
        assert C.tier_of(n, s.size) == tier
        assert C.repeated_keys(d, chunk).size and C.repeated_keys(s, chunk).size, (name, i)
        # a placement that is not stable in edge id is a different answer for this molecule
        csr = graph_ref.csr_ref(s, d, n)
        for rp, key in (("in_rowptr", "in_src"), ("in_rowptr", "in_eid"),
                        ("out_rowptr", "out_dst"), ("out_rowptr", "out_inslot")):
            assert not np.array_equal(C.reverse_rows(csr[rp], csr[key]), csr[key]), (name, i, key)
        if tier in "LS":  # rows_from_counts: the carry into the 2nd and 3rd 256-row block matters
            T = K["kCsrThreads"]
            assert n > 2 * T
            for rp in ("in_rowptr", "out_rowptr"):
                cnt = np.diff(csr[rp])
                assert cnt[:T].any() and cnt[T:2 * T].any() and cnt[2 * T:3 * T].any()


def test_repeated_keys_and_reverse_rows_helpers():
    # key 4: twice in round 0 and once in round 1; key 9: twice in round 1 only; key 2: once each
    keys = [4, 4, 2, 1, 4, 9, 9, 2]
    assert C.repeated_keys(keys, 4).tolist() == [4]
    assert C.repeated_keys(keys, 8).tolist() == []
    out = C.reverse_rows([0, 3, 3, 5], np.array([10, 11, 12, 20, 21]))
    assert out.tolist() == [12, 11, 10, 21, 20]


def test_trip_cases_exceed_the_persistent_grids():
    tb, tl, tm = (C.case(n).tiers() for n in C.TRIP_CASES)
    assert tb.count("B") > BIGWAVE_GRID and tl.count("L") > CSR_GRID
    assert tm.count("B") > BIGWAVE_GRID and tm.count("L") > CSR_GRID and tm.count("W") > 0
    # class L's second list is filled by class B's kernel: its entries pass through both lists
    assert len(C.case("trips_L").bnn) > CSR_GRID


@pytest.mark.parametrize("name", C.SCAN_CASES + ("scan_second_trip",))
def test_scan_cases(name):
    c = C.case(name)
    B, T = len(c.bnn), K["kScanTile"]
    assert c.bnn.max() <= 3 and c.bnn.sum() > 0
    if name == "scan_second_trip":  # more than 256 tile sums: scan2_sums_single's second trip
        assert B == 256 * T + 5 and -(-B // T) > 256
        assert 1.5 < c.bnn.mean() < 2.5 and 2 < c.bne.mean() < 4
    else:
        assert B == int(name.split("_")[1])
    if B >= 8:
        assert c.bnn[0] == 0 and c.bnn[-1] == 0
        for edge in range(T, B, T):
            assert c.bnn[edge - 1] == 0 and c.bnn[edge] == 0
        run = np.flatnonzero(c.bnn == 0)
        assert np.any(run[4:] - run[:-4] == 4)  # five consecutive empty molecules


def test_scan_sizes_straddle_the_tile():
    T = K["kScanTile"]
    assert {1, 2, T - 1, T, T + 1, 2 * T + 1} == set(C.SCAN_SIZES)
    e = C.case("all_empty")
    assert len(e.bnn) > 0 and e.bnn.sum() == 0 and e.bne.sum() == 0
    assert len(C.case("no_molecules").bnn) == 0


def test_isolated_case_counts():
    c = C.case("isolated")
    want = {t: k for t, (_, _, k) in C.ISOLATED.items()}
    assert len(set(want.values())) == 4
    got = {}
    for i in c.subjects:
        n, s, d = c.molecule(i)
        got[C.tier_of(n, s.size)] = int((np.bincount(d, minlength=n) == 0).sum())
    assert got == want
    ref = C.oracle(*c.args())
    assert ref["zero_in_degree"] == sum(want.values())  # nothing else in the batch adds to it


@pytest.mark.parametrize("tier", "WBLS")
def test_bad_cases(tier):
    bad, i, good = C.bad_case(tier)
    n, s, d = bad.molecule(i)
    assert C.tier_of(n, s.size) == tier
    invalid = (s < 0) | (s >= n) | (d < 0) | (d >= n)
    assert invalid.sum() == 3 and not invalid[0] and not invalid[-1]
    assert {-1, 2 ** 31 - 1} <= set(s[invalid].tolist()) and n in d[invalid].tolist()
    assert np.array_equal(bad.bnn, good.bnn) and np.array_equal(bad.bne, good.bne)
    same = np.ones(bad.src_l.size, bool)
    same[bad.edge_off[i]:bad.edge_off[i + 1]] = False
    assert np.array_equal(bad.src_l[same], good.src_l[same])
    assert np.array_equal(bad.dst_l[same], good.dst_l[same])
    gn = np.repeat(good.bnn, good.bne)
    assert np.all((good.src_l >= 0) & (good.src_l < gn) & (good.dst_l >= 0) & (good.dst_l < gn))


def test_all_classes_case_has_zero_in_degree_atoms():
    """recollate() twice must leave the zero-in-degree COUNT unchanged: it has to be non-zero."""
    assert C.oracle(*C.case("all_classes").args())["zero_in_degree"] > 0


# ------------------------------------------------------------------ node-group plan inputs
def _plan_ref_loop(node_offsets, in_rowptr):
    """node_group_plan_ref restated group by group (the form it had before it was vectorised)."""
    ga = K["kNodeGroupAtoms"]
    no, rp = np.asarray(node_offsets, np.int64), np.asarray(in_rowptr, np.int64)
    N = int(no[-1])
    G = -(-N // ga)
    starts = [int(no[np.searchsorted(no, g * ga, side="right") - 1]) for g in range(G)] + [N]
    kinds, fwd, bwd = [0] * G, set(), set()
    for g in range(G):
        a0, a1 = starts[g], starts[g + 1]
        if a1 <= a0:
            continue
        atoms, edges = a1 - a0, rp[a1] - rp[a0]
        fits = atoms <= K["kPlanWinAtoms"] and edges <= K["kPlanEdgeCap"]
        big = atoms <= K["kPlanBigAtoms"] and edges <= K["kPlanBigEdgeCap"]
        dmax = int(np.max(rp[a0 + 1:a1 + 1] - rp[a0:a1]))
        kinds[g] = (1 if fits and dmax <= K["kPlanDegCap"] else 0) | (2 if fits else 0) | (4 if big else 0)
        if not kinds[g] & 1:
            fwd.add(g)
        if not kinds[g] & 2:
            bwd.add(g)
    return starts, kinds, fwd, bwd


@pytest.mark.parametrize("name", ["caps", "G1", "G1023", "G1025"])
def test_vectorised_plan_oracle_equals_the_loop(name):
    no, rp = C.plan_case(name)
    starts, kinds, fwd, bwd = C.plan_ref(no, rp)
    s2, k2, f2, b2 = _plan_ref_loop(no, rp)
    assert starts.dtype == np.int32 and kinds.dtype == np.int32
    assert starts.tolist() == s2 and kinds.tolist() == k2 and fwd == f2 and bwd == b2


def _groups(no, rp):
    """(atoms, in-edges, max in-degree, kind) of every non-empty group."""
    starts, kinds, _, _ = C.plan_ref(no, rp)
    starts, rp = starts.astype(np.int64), np.asarray(rp, np.int64)
    live = np.flatnonzero(np.diff(starts) > 0)
    a0, a1 = starts[live], starts[live + 1]
    dmax = np.maximum.reduceat(np.diff(rp), a0)
    return list(zip((a1 - a0).tolist(), (rp[a1] - rp[a0]).tolist(), dmax.tolist(),
                    kinds[live].tolist()))


def test_plan_caps_case_straddles_every_cap():
    no, rp = C.plan_case("caps")
    wa, ec, dc, ba, bec = (K[k] for k in ("kPlanWinAtoms", "kPlanEdgeCap", "kPlanDegCap",
                                          "kPlanBigAtoms", "kPlanBigEdgeCap"))
    gs = _groups(no, rp)
    has = lambda pred: any(pred(*g) for g in gs)
    # (atoms, edges, dmax, kind): each probe with the other quantities inside their caps
    assert has(lambda a, e, d, k: a == wa and e < ec and d <= dc and k == 7)
    assert has(lambda a, e, d, k: a == wa + 1 and e < ec and d <= dc and k == 4)
    assert has(lambda a, e, d, k: a == ba and e < bec and k == 4)
    assert has(lambda a, e, d, k: a == ba + 1 and e < bec and k == 0)
    assert has(lambda a, e, d, k: a <= wa and e == ec and d <= dc and k == 7)
    assert has(lambda a, e, d, k: a <= wa and e == ec + 1 and d <= dc and k == 4)
    assert has(lambda a, e, d, k: a <= ba and e == bec and k == 4)
    assert has(lambda a, e, d, k: a <= ba and e == bec + 1 and k == 0)
    assert has(lambda a, e, d, k: a < wa and e < ec and d == dc and k == 7)
    assert has(lambda a, e, d, k: a < wa and e < ec and d == dc + 1 and k == 6)
    # a molecule spanning >= 3 multiples of the group size: empty groups; and empty molecules
    # exactly where a group starts
    ga = K["kNodeGroupAtoms"]
    starts = C.plan_ref(no, rp)[0]
    assert np.any(np.diff(starts) == 0)
    sizes = np.diff(no)
    assert np.any(sizes // ga >= 3)
    empty_at = no[:-1][sizes == 0]
    assert np.intersect1d(empty_at, starts).size >= 5 and np.all(empty_at % ga == 0)


def test_plan_group_counts():
    ga = K["kNodeGroupAtoms"]
    count = lambda name: -(-int(C.plan_case(name)[0][-1]) // ga)
    for G in (1, 1023, 1024, 1025, 65536, 65537):
        assert count(f"G{G}") == G
        no, rp = C.plan_case(f"G{G}")
        _, kinds, fwd, bwd = C.plan_ref(no, rp)
        if G > 1:  # every kind of group and both lists occur
            assert {0, 4, 6, 7} <= set(kinds.tolist()) and fwd and bwd and fwd != bwd
    # R = groups per thread of node_group_lists_kernel: 64 -> 65 is the first re-read
    assert -(-65536 // 1024) == 64 and -(-65537 // 1024) == 65


def test_plan_reread_case():
    """R >= 129: two re-read rounds per thread.  On each list some thread has entries in the
    first, a middle and the last 64-block of its range, some thread has them only in its last
    block, and some thread that owns groups has none."""
    no, rp = C.plan_case("reread")
    G = -(-int(no[-1]) // K["kNodeGroupAtoms"])
    R = -(-G // 1024)
    assert G == C.PLAN_REREAD_GROUPS and R >= 129
    last = (R - 1) // 64
    assert last >= 2
    _, _, fwd, bwd = C.plan_ref(no, rp)
    assert bwd < fwd
    for lst in (fwd, bwd):
        g = np.array(sorted(lst))
        thread, block = g // R, (g % R) // 64
        blocks = {}
        for t, b in zip(thread.tolist(), block.tolist()):
            blocks.setdefault(t, set()).add(b)
        assert any(0 in b and last in b and any(0 < x < last for x in b) for b in blocks.values())
        assert any(b == {last} for b in blocks.values())
        owners = -(-G // R)
        assert len(blocks) < owners - 1
