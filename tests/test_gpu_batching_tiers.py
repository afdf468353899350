"""Device batching (csrc/batch_csr.hip) against oracle/graph_ref.py, bit for bit, at every size
class of a molecule, on both sides of every class limit, with keys repeated inside and across
placement chunks, with more listed molecules than the persistent grids, through every pass of
the offset scans and of the node-group list builder.  The inputs come from _batching_cases.py;
test_batching_cases_cpu.py checks that they hold the hard cases these comparisons rely on.

Wall time per test on an MI355X, host oracle included: under 0.3 s each (the largest inputs:
trips_mixed 0.12 s, scan_second_trip 0.05 s, the R = 129 plan 0.05 s)."""
import numpy as np
import pytest
import torch

import _batching_cases as C
from mvml_gat import batching

pytestmark = pytest.mark.gpu
DEV = C.DEV


def _check(name):
    c = C.case(name)
    out = C.build_direct(*c.args())
    return c, out, C.assert_matches_oracle(out, *c.args())


# ------------------------------------------------------------------ 3a class limits, neighbours
@pytest.mark.parametrize("name", C.BOUNDARY_CASES)
def test_class_limits(name):
    """Molecules exactly at and one above every class limit, beside 0-atom, 1-atom and other
    at-limit molecules in one workgroup: an off-by-one in the routing overruns an LDS slice
    into the neighbour's."""
    _check(name)


# ------------------------------------------------------------------ 3b repeated keys, carry
@pytest.mark.parametrize("name", C.REPEAT_CASES)
def test_repeated_keys(name):
    """A hub of degree above the placement chunk and a random multigraph per class: ranks
    inside a chunk, cursors across chunks, and (L, S) the row scan's carry across 256-row
    blocks."""
    _check(name)


# ------------------------------------------------------------------ 3c persistent trips
@pytest.mark.parametrize("name", C.TRIP_CASES)
def test_persistent_trips(name):
    """More class-B molecules than build_csr_bigwave_kernel's grid and more class-L ones than
    build_csr_kernel's: the `li += gridDim.x` loops take a second trip."""
    _check(name)


# ------------------------------------------------------------------ 3d offset scans
@pytest.mark.parametrize("name", C.SCAN_CASES + ("scan_second_trip",))
def test_offset_scans(name):
    """One tile, the tile boundary, several tiles, and more than 256 tile sums; empty molecules
    first, last, on both sides of every tile boundary and in a run."""
    _check(name)


@pytest.mark.parametrize("name", ["all_empty", "no_molecules"])
def test_nothing_to_build(name):
    c, out, _ = _check(name)
    assert out["in_rowptr"].tolist() == [0] and out["out_rowptr"].tolist() == [0]
    assert out["status_flags"].tolist() == [0, 0]
    graphs = [batching.MolGraph(0, [], []) for _ in range(len(c.bnn))]
    g = batching.batch(graphs).to(DEV)
    torch.cuda.synchronize()
    assert g.in_rowptr.cpu().tolist() == [0] and g.out_rowptr.cpu().tolist() == [0]
    assert g.node_offsets.cpu().tolist() == [0] * (len(c.bnn) + 1)
    assert g.has_zero_in_degree is False and g.num_node_groups == 0


# ------------------------------------------------------------------ 3e status flag 0 is a count
def test_zero_in_degree_count_per_class():
    """3, 5, 7 and 11 atoms without an in-edge in the class W, B, L and S molecule: the flag is
    their sum, so each class's kernel counted its own exactly."""
    c, out, ref = _check("isolated")
    assert int(out["status_flags"][0]) == sum(k for _, _, k in C.ISOLATED.values()) == 26


# ------------------------------------------------------------------ 3f ids outside the molecule
@pytest.mark.parametrize("tier", "WBLS")
def test_bad_ids_per_class(tier):
    """Three edges with an id outside their molecule (-1, n, 2^31 - 1) in the class's molecule:
    counted exactly, rejected by BatchedMolGraph.to, and skipped without touching anything of
    the other molecules (the kernels skip such edges by design)."""
    bad, i, good = C.bad_case(tier)
    out = C.build_direct(*bad.args())
    assert int(out["status_flags"][1]) == 3
    with pytest.raises(ValueError, match=r"\b3 edges"):
        batching.from_arrays(*bad.args()).to(DEV)
    ref = C.oracle(*good.args())
    e0, e1 = int(bad.edge_off[i]), int(bad.edge_off[i + 1])
    others = np.ones(bad.src_l.size, bool)
    others[e0:e1] = False
    for k in C.INDEX_KEYS:
        # offsets, node_graph and the row starts of every molecule but the bad one do not
        # depend on its edges' ids; its own rows (fewer edges counted) are left out
        if k in C.EDGE_KEYS:
            np.testing.assert_array_equal(out[k][others], ref[k][others], err_msg=k)
            assert not np.any(out[k][others] == C.SENTINEL), k
        elif k.endswith("rowptr"):
            n0, n1 = (int(x) for x in ref["node_offsets"][i:i + 2])
            rows = np.ones(out[k].size, bool)
            rows[n0 + 1:n1] = False  # row n0 starts at e0, row n1 (the next molecule) at e1
            np.testing.assert_array_equal(out[k][rows], ref[k][rows], err_msg=k)
            assert not np.any(out[k] == C.SENTINEL), k
        else:
            np.testing.assert_array_equal(out[k], ref[k], err_msg=k)


# ------------------------------------------------------------------ 3g recollate
def test_recollate_all_classes():
    """recollate() into sentinel-filled buffers is bitwise the first build, for a batch with
    all four classes, and the zero-in-degree count does not accumulate over recollations (the
    first scan kernel re-zeroes the flags)."""
    c = C.case("all_classes")
    ref = C.oracle(*c.args())
    g = batching.from_arrays(*c.args()).to(DEV)
    keys = C.INDEX_KEYS + ("node_groups",)
    first = {k: getattr(g, k).clone() for k in keys}
    flags = g._dev["_inputs"][4]
    assert flags.cpu().tolist() == [ref["zero_in_degree"], 0] and g.has_zero_in_degree is True
    G = g.num_node_groups
    for _ in range(2):
        for k in keys:
            getattr(g, k).fill_(C.SENTINEL)
        g.recollate()
        torch.cuda.synchronize()
        for k in C.INDEX_KEYS:
            assert torch.equal(getattr(g, k), first[k]), k
        a, b = first["node_groups"].cpu().numpy(), g.node_groups.cpu().numpy()
        np.testing.assert_array_equal(a[:2 * G + 3], b[:2 * G + 3])
        for base, n in ((2 * G + 3, int(a[2 * G + 1])), (3 * G + 3, int(a[2 * G + 2]))):
            np.testing.assert_array_equal(a[base:base + n], b[base:base + n])
        assert flags.cpu().tolist() == [ref["zero_in_degree"], 0]
        assert bool(flags[0].item() > 0) is g.has_zero_in_degree
    for k in C.INDEX_KEYS:
        np.testing.assert_array_equal(first[k].cpu().numpy(), ref[k], err_msg=k)


# ------------------------------------------------------------------ 3h node-group plan, directly
@pytest.mark.parametrize("name", C.PLAN_CASE_NAMES)
def test_node_group_plan_direct(name):
    """mvml_build_node_groups on host-made node_offsets / in_rowptr (no CSR build): groups on
    both sides of every cap, empty groups, empty molecules at group starts, one to several
    list-scan chunks, R = 64 -> 65 groups per thread (the first re-read of the flags) and
    R = 129 (two re-reads, fallback groups in the first, a middle and the last 64-block)."""
    no, rp = C.plan_case(name)
    G, plan = C.build_plan_direct(no, rp)
    C.assert_plan_matches_oracle(G, plan, no, rp)
