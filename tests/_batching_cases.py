"""Inputs and driver for the device-batching tests (csrc/batch_csr.hip against oracle/graph_ref.py).

Every case is written in terms of the size-class limits parsed from the kernel source
(tier_constants), so the cases follow the code if a limit moves.  The CPU conditions on these
inputs are in test_batching_cases_cpu.py, the GPU comparisons in test_gpu_batching_tiers.py.

Size classes of one molecule of n atoms and ne directed edges (mvml_build_csr):
  W  build_csr_wave_kernel     n <= kWaveMolAtoms and ne <= kWaveMolEdges
  B  build_csr_bigwave_kernel  otherwise, n <= kBigMolAtoms and ne <= kBigMolEdges
  L  build_csr_kernel, histogram in LDS        otherwise, n <= kLdsNodes
  S  build_csr_kernel, histogram in workspace  n > kLdsNodes
"""
import functools
import os
import re

import numpy as np

from oracle import graph_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mvml-mpi_amd", "csrc")
SENTINEL = -7
INDEX_KEYS = ("node_offsets", "edge_offsets", "src", "dst", "node_graph", "in_rowptr", "in_src",
              "in_eid", "out_rowptr", "out_dst", "out_inslot")
EDGE_KEYS = ("src", "dst", "in_src", "in_eid", "out_dst", "out_inslot")
CONSTANT_NAMES = ("kWaveMolAtoms", "kWaveMolEdges", "kBigMolAtoms", "kBigMolEdges", "kLdsNodes",
                  "kScanTile", "kCsrThreads", "kNodeGroupAtoms", "kPlanWinAtoms", "kPlanEdgeCap",
                  "kPlanDegCap", "kPlanBigAtoms", "kPlanBigEdgeCap")
WAVE_CHUNK = 64  # edges per placement round of the one-wave-per-molecule kernels (the wave size)


# ------------------------------------------------------------------ constants from the source
@functools.lru_cache(maxsize=None)
def tier_constants():
    """{name: int} of CONSTANT_NAMES, read from the `constexpr int k... = ...;` lines of
    batch_csr.hip and common.h (a value may be a product of earlier constants: kScanTile)."""
    vals = {}
    for fn in ("common.h", "batch_csr.hip"):
        with open(os.path.join(CSRC, fn)) as f:
            text = f.read()
        for m in re.finditer(r"constexpr\s+int\s+(k\w+)\s*=\s*([^;]+);", text):
            prod = 1
            for tok in m.group(2).split("*"):
                tok = tok.strip()
                if re.fullmatch(r"\d+", tok):
                    prod *= int(tok)
                elif tok in vals:
                    prod *= vals[tok]
                else:
                    prod = None
                    break
            if prod is not None:
                vals[m.group(1)] = prod
    return {k: vals[k] for k in CONSTANT_NAMES}


def tier_of(n, ne):
    K = tier_constants()
    if n <= K["kWaveMolAtoms"] and ne <= K["kWaveMolEdges"]:
        return "W"
    if n <= K["kBigMolAtoms"] and ne <= K["kBigMolEdges"]:
        return "B"
    return "L" if n <= K["kLdsNodes"] else "S"


def chunk_of(tier):
    """Edges ranked together in one placement round of the class's kernel."""
    return WAVE_CHUNK if tier in "WB" else tier_constants()["kCsrThreads"]


# ------------------------------------------------------------------ molecule makers
def _i32(a):
    return np.ascontiguousarray(a, dtype=np.int32)


def chain(n, self_loops=True):
    """Path 0-1-...-(n-1) in mol_to_bigraph order: (i -> i+1), (i+1 -> i) per bond, then one
    self-loop per atom.  2 (n - 1) edges, + n with self-loops."""
    a = np.arange(max(n - 1, 0), dtype=np.int32)
    src = np.empty(2 * a.size, np.int32)
    dst = np.empty(2 * a.size, np.int32)
    src[0::2], dst[0::2] = a, a + 1
    src[1::2], dst[1::2] = a + 1, a
    if self_loops:
        loop = np.arange(n, dtype=np.int32)
        src, dst = np.concatenate([src, loop]), np.concatenate([dst, loop])
    return _i32(src), _i32(dst)


def multi(n, ne, seed):
    """Random directed multigraph: exactly ne edges over n atoms, duplicates and self-loops
    allowed (how ne passes an edge limit with few atoms)."""
    assert n > 0 or ne == 0
    rng = np.random.default_rng(seed)
    if ne == 0:
        return np.zeros(0, np.int32), np.zeros(0, np.int32)
    return _i32(rng.integers(0, n, ne)), _i32(rng.integers(0, n, ne))


def hub(n, ne, k, seed):
    """As multi, but atom h receives exactly k in-edges and emits exactly k out-edges, at
    positions drawn over the whole edge list: the key h repeats inside a placement chunk and
    again in later chunks."""
    assert n >= 2 and 2 * k <= ne
    rng = np.random.default_rng(seed)
    h = int(rng.integers(0, n))
    src = rng.integers(0, n - 1, ne)
    dst = rng.integers(0, n - 1, ne)
    src += src >= h  # every other edge avoids h
    dst += dst >= h
    pos = rng.permutation(ne)
    dst[pos[:k]] = h
    src[pos[k:2 * k]] = h
    return _i32(src), _i32(dst)


def with_isolated(n, ne, k, seed):
    """n atoms of which the last k have no in-edge and every other one has at least one (a
    self-loop on each, then random edges among them): exactly k zero-in-degree atoms."""
    m = n - k
    assert m > 0 and ne >= m
    s, d = multi(m, ne - m, seed)
    loop = np.arange(m, dtype=np.int32)
    return _i32(np.concatenate([loop, s])), _i32(np.concatenate([loop, d]))


def small(seed):
    """A filler molecule of 1-20 atoms (class W)."""
    rng = np.random.default_rng(1000 + seed)
    n = int(rng.integers(1, 21))
    return (n,) + multi(n, int(rng.integers(1, 3 * n + 2)), 2000 + seed)


EMPTY = (0, np.zeros(0, np.int32), np.zeros(0, np.int32))


def one_atom(ne=2):
    return (1, np.zeros(ne, np.int32), np.zeros(ne, np.int32))


def mol(maker, n, *args):
    return (n,) + maker(n, *args)


# ------------------------------------------------------------------ cases
class Case:
    """One batch.  names: the size classes the case is about; subjects: indices of the molecules
    whose properties the CPU conditions check (the fillers around them are not)."""

    def __init__(self, bnn, bne, src_l, dst_l, names="", subjects=(), limits=()):
        self.bnn = np.ascontiguousarray(bnn, dtype=np.int64)
        self.bne = np.ascontiguousarray(bne, dtype=np.int64)
        self.src_l, self.dst_l = _i32(src_l), _i32(dst_l)
        assert self.src_l.shape == self.dst_l.shape == (int(self.bne.sum()),)
        self.names, self.subjects, self.limits = names, tuple(subjects), tuple(limits)
        self.edge_off = np.concatenate([[0], np.cumsum(self.bne)])

    @classmethod
    def of(cls, mols, **kw):
        mols = list(mols)
        for n, s, d in mols:
            assert s.shape == d.shape
        cat = lambda i: (np.concatenate([m[i] for m in mols]) if mols else np.zeros(0, np.int32))
        return cls([m[0] for m in mols], [m[1].size for m in mols], cat(1), cat(2), **kw)

    def molecule(self, i):
        a, b = self.edge_off[i], self.edge_off[i + 1]
        return int(self.bnn[i]), self.src_l[a:b], self.dst_l[a:b]

    def tiers(self):
        return [tier_of(int(n), int(e)) for n, e in zip(self.bnn, self.bne)]

    def args(self):
        return self.bnn, self.bne, self.src_l, self.dst_l


def limit_pairs():
    """{limit name: ((n, ne) at the limit, (n, ne) one above it)}: atom limits with the edge
    count inside the class, edge limits with the atom count inside it."""
    K = tier_constants()
    wa, we, ba, be, la = (K[k] for k in ("kWaveMolAtoms", "kWaveMolEdges", "kBigMolAtoms",
                                         "kBigMolEdges", "kLdsNodes"))
    return {
        "W atoms": ((wa, we), (wa + 1, min(300, we))),
        "W edges": ((wa, we), (min(100, wa), we + 1)),
        "B atoms": ((ba, be), (ba + 1, min(2048, be))),
        "B edges": ((ba, be), (min(600, ba), be + 1)),
        "L atoms": ((la, 9000), (la + 1, 9000)),
    }


def _interleave(subjects, seed):
    """[subject, 1-atom, 0-atom, small, subject, ...]: returns (mols, indices of the subjects)."""
    mols, idx = [small(seed)], []
    for j, m in enumerate(subjects):
        idx.append(len(mols))
        mols += [m, one_atom(), EMPTY, small(seed + 1 + j)]
    return mols, idx


def _case_w_full():
    (n, ne), _ = limit_pairs()["W atoms"]
    return Case.of([mol(multi, n, ne, 10 + i) for i in range(8)], names="W", subjects=range(8),
                   limits=("W atoms", "W edges"))


def _case_w_limits():
    P = limit_pairs()
    at = P["W atoms"][0]
    # workgroups of four: [small, 129-atom, 1, 0] [small, 513-edge, 1, 0] [small, at, 1, 0] ...
    subj = [mol(multi, *P["W atoms"][1], 21), mol(multi, *P["W edges"][1], 22),
            mol(multi, *at, 23), mol(multi, *at, 24), mol(multi, *P["W atoms"][1], 25),
            mol(multi, *at, 26)]
    mols, idx = _interleave(subj, 20)
    mols += [mol(multi, *at, 27), mol(multi, *P["W edges"][1], 28), mol(multi, *at, 29)]
    return Case.of(mols, names="WB", subjects=idx, limits=("W atoms", "W edges"))


def _case_b_limits():
    P = limit_pairs()
    subj = [mol(multi, *P["B atoms"][0], 31), mol(multi, *P["B atoms"][1], 32),
            mol(multi, *P["B edges"][1], 33), mol(multi, *P["B atoms"][0], 34)]
    mols, idx = _interleave(subj, 30)
    return Case.of(mols, names="WBL", subjects=idx, limits=("B atoms", "B edges"))


def _case_l_limits():
    P = limit_pairs()
    subj = [mol(multi, *P["L atoms"][0], 41), mol(multi, *P["L atoms"][1], 42),
            mol(multi, *P["L atoms"][0], 43)]
    mols, idx = _interleave(subj, 40)
    return Case.of(mols, names="WLS", subjects=idx, limits=("L atoms",))


def _case_all_classes():
    P = limit_pairs()
    pairs = [p for at, above in P.values() for p in (at, above)]
    mols = [mol(multi, n, ne, 50 + i) for i, (n, ne) in enumerate(pairs)]
    mols += [small(60 + i) for i in range(9)] + [EMPTY, one_atom(), EMPTY]
    order = np.random.default_rng(5).permutation(len(mols))
    mols = [mols[i] for i in order]
    return Case.of(mols, names="WBLS", limits=tuple(P))


REPEAT_SHAPES = {  # class: (hub n, ne, hub degree), (multi n, ne)
    "W": ((120, 500, 100), (100, 400)),
    "B": ((700, 3000, 300), (500, 2500)),
    "L": ((1500, 6000, 700), (2000, 7000)),
    "S": ((4500, 12000, 700), (5000, 11000)),
}


def _case_repeats(tier):
    (hn, he, hk), (mn, me) = REPEAT_SHAPES[tier]
    seed = 70 + 10 * "WBLS".index(tier)
    mols = [small(seed), small(seed + 1), mol(hub, hn, he, hk, seed + 2), small(seed + 3), EMPTY,
            mol(multi, mn, me, seed + 4), small(seed + 5)]
    return Case.of(mols, names="W" + tier if tier != "W" else "W", subjects=(2, 5))


def _case_trips(kind):
    K = tier_constants()
    b = mol(chain, K["kWaveMolAtoms"] + 1)            # class B by its atoms
    l = mol(chain, K["kBigMolAtoms"] + 1, False)      # class L by its atoms
    nb, nl = 2048 + 52, 512 + 8                       # more than the persistent grids
    if kind == "B":
        return Case.of([b] * nb, names="B")
    if kind == "L":
        return Case.of([l] * nl, names="L")
    mols = []
    for i in range(nb):  # 4 : 1 : 1, the L molecules spread over the first part of the batch
        mols.append(b)
        if i % 4 == 0 and i // 4 < nl:
            mols.append(l)
        if i % 4 == 2:
            mols.append(small(i % 17))
    return Case.of(mols, names="WBL")


def tiny_batch(B, seed, empties=True):
    """B molecules of 0-3 atoms and 0-6 edges.  With `empties`, 0-atom molecules sit at the
    first and last position, on both sides of every scan-tile boundary and in a run of five."""
    rng = np.random.default_rng(seed)
    T = tier_constants()["kScanTile"]
    n = rng.integers(1, 4, B)
    if empties and B >= 2:
        n[0] = 0
    if empties and B >= 8:
        n[B - 1] = 0
        edge = np.arange(T, B, T)
        n[edge] = 0
        n[edge - 1] = 0
        n[B // 2:B // 2 + 5] = 0
    ne = rng.integers(0, 7, B) * (n > 0)
    nrep = np.repeat(n, ne)
    src = (rng.random(nrep.size) * nrep).astype(np.int32)
    dst = (rng.random(nrep.size) * nrep).astype(np.int32)
    return Case(n, ne, src, dst, names="W")


SCAN_SIZES = (1, 2, 1023, 1024, 1025, 2049)


def scan_second_trip_size():
    return 256 * tier_constants()["kScanTile"] + 5


ISOLATED = {"W": (100, 300, 3), "B": (600, 2000, 5), "L": (2500, 6000, 7), "S": (4200, 9000, 11)}


def _case_isolated():
    mols = [small(90)]
    for i, t in enumerate("SWLB"):
        n, ne, k = ISOLATED[t]
        mols += [mol(with_isolated, n, ne, k, 91 + i), (3,) + chain(3)]
    return Case.of(mols, names="WBLS", subjects=(1, 3, 5, 7))


BAD_SHAPES = {"W": (100, 400), "B": (500, 2500), "L": (2000, 7000), "S": (4500, 10000)}


def bad_case(tier):
    """A batch whose class-`tier` molecule carries 3 edges with an id outside the molecule (-1,
    n, 2^31 - 1) among valid ones.  Returns (case, index of that molecule, the same case with
    those 3 edges replaced by valid ones, for the oracle)."""
    n, ne = BAD_SHAPES[tier]
    seed = 110 + "WBLS".index(tier)
    other = "B" if tier != "B" else "L"
    on, oe = BAD_SHAPES[other]
    s, d = multi(n, ne, seed)
    good = [small(seed), mol(multi, on, oe, seed + 20), (n, s, d), small(seed + 1), EMPTY,
            small(seed + 2)]
    bs, bd = s.copy(), d.copy()
    bs[5], bd[ne // 2], bs[ne - 2] = -1, n, 2 ** 31 - 1
    bad = list(good)
    bad[2] = (n, bs, bd)
    return (Case.of(bad, names=tier + other + "W", subjects=(2,)), 2,
            Case.of(good, names=tier + other + "W"))


_CASES = {
    "w_full": _case_w_full, "w_limits": _case_w_limits, "b_limits": _case_b_limits,
    "l_limits": _case_l_limits, "all_classes": _case_all_classes,
    "repeats_W": lambda: _case_repeats("W"), "repeats_B": lambda: _case_repeats("B"),
    "repeats_L": lambda: _case_repeats("L"), "repeats_S": lambda: _case_repeats("S"),
    "trips_B": lambda: _case_trips("B"), "trips_L": lambda: _case_trips("L"),
    "trips_mixed": lambda: _case_trips("mixed"),
    "isolated": _case_isolated,
    "all_empty": lambda: Case(np.zeros(37), np.zeros(37), [], [], names="W"),
    "no_molecules": lambda: Case([], [], [], [], names=""),
    "scan_second_trip": lambda: tiny_batch(scan_second_trip_size(), 7),
}
_CASES.update({f"scan_{B}": (lambda B=B: tiny_batch(B, B)) for B in SCAN_SIZES})
BOUNDARY_CASES = ("w_full", "w_limits", "b_limits", "l_limits", "all_classes")
REPEAT_CASES = ("repeats_W", "repeats_B", "repeats_L", "repeats_S")
TRIP_CASES = ("trips_B", "trips_L", "trips_mixed")
SCAN_CASES = tuple(f"scan_{B}" for B in SCAN_SIZES)
CASE_NAMES = tuple(_CASES)


@functools.lru_cache(maxsize=4)
def case(name):
    return _CASES[name]()


# ------------------------------------------------------------------ properties of the inputs
def repeated_keys(keys, chunk):
    """Keys that occur at least twice inside one `chunk`-edge placement round and in at least two
    different rounds: where a wrong rank, `last` or cursor advance changes the placement."""
    keys = np.asarray(keys, dtype=np.int64)
    rounds = np.arange(keys.size) // chunk
    nr = int(rounds[-1]) + 1 if keys.size else 1
    pair, cnt = np.unique(keys * nr + rounds, return_counts=True)
    twice = np.unique(pair[cnt >= 2] // nr)
    k, nrounds = np.unique(pair // nr, return_counts=True)
    return np.intersect1d(twice, k[nrounds >= 2])


def reverse_rows(rowptr, arr):
    """arr with the entries of every CSR row in reverse order (a non-stable placement)."""
    rowptr = np.asarray(rowptr, dtype=np.int64)
    row = np.repeat(np.arange(rowptr.size - 1), np.diff(rowptr))
    slot = np.arange(arr.size)
    return arr[rowptr[row] + rowptr[row + 1] - 1 - slot]


# ------------------------------------------------------------------ node-group plan inputs
def plan_from(sizes, deg):
    """Synthetic inputs of mvml_build_node_groups: node_offsets int64[B+1] from the molecule
    sizes, in_rowptr int32[N+1] from the in-degree of every atom."""
    sizes = np.asarray(sizes, dtype=np.int64)
    no = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    deg = np.asarray(deg, dtype=np.int64)
    assert deg.size == no[-1]
    return no, np.concatenate([[0], np.cumsum(deg)]).astype(np.int32)


def plan_caps_probes():
    """(atoms, in-degrees) of one-molecule groups on both sides of every cap of the plan, each
    with the other quantities inside their caps; then a molecule spanning 5 multiples of the
    group size (empty groups)."""
    K = tier_constants()
    wa, ec, dc, ba, bec = (K[k] for k in ("kPlanWinAtoms", "kPlanEdgeCap", "kPlanDegCap",
                                          "kPlanBigAtoms", "kPlanBigEdgeCap"))
    full = lambda n, d: np.full(n, d, np.int64)

    def total(n, e):  # n atoms, e in-edges in all, in-degrees differing by at most one
        d = full(n, e // n)
        d[:e % n] += 1
        return d

    def one(n, d, peak):
        v = full(n, d)
        v[n // 3] = peak
        return v
    lo = min(3, dc)
    return [
        (wa, full(wa, lo)), (wa + 1, full(wa + 1, lo)),            # 128 / 129 atoms
        (ba, full(ba, lo)), (ba + 1, full(ba + 1, lo)),            # 512 / 513 atoms
        (wa, total(wa, ec)), (wa, total(wa, ec + 1)),              # 512 / 513 in-edges
        (ba, total(ba, bec)), (ba, total(ba, bec + 1)),            # 2432 / 2433 in-edges
        (100, one(100, lo, dc)), (100, one(100, lo, dc + 1)),      # in-degree 5 / 6
        (5 * K["kNodeGroupAtoms"] - 20, full(5 * K["kNodeGroupAtoms"] - 20, lo)),
    ]


def _plan_caps():
    """Every probe starts on a multiple of the group size, after two empty molecules, and is
    followed by a filler molecule that ends on one and holds the multiple after the probe: the
    probe is then a group of its own."""
    ga = tier_constants()["kNodeGroupAtoms"]
    sizes, degs, pos = [], [], 0
    for n, d in plan_caps_probes():
        assert pos % ga == 0
        fill = -(pos + n) % ga + ga
        sizes += [0, 0, n, fill]
        degs += [d, np.full(fill, 2, np.int64)]
        pos += n + fill
    sizes += [0]
    return plan_from(sizes, np.concatenate(degs))


def _plan_random(G, seed):
    """Exactly G groups of random 0-150-atom molecules; in-degrees 1-4, three atoms in a
    thousand 6 or 7 (above the forward cap)."""
    rng = np.random.default_rng(seed)
    ga = tier_constants()["kNodeGroupAtoms"]
    N = (G - 1) * ga + int(rng.integers(1, ga + 1))
    sizes = rng.integers(0, 151, N // 60 + 16)
    off = np.cumsum(sizes)
    keep = int(np.searchsorted(off, N, side="left"))  # molecules wholly below N, then the rest
    sizes = np.concatenate([sizes[:keep], [N - (off[keep - 1] if keep else 0)], [0]])
    deg = rng.integers(1, 5, N)
    high = rng.random(N) < 0.003
    deg[high] = rng.integers(6, 8, int(high.sum()))
    return plan_from(sizes, deg)


PLAN_REREAD_GROUPS = 128 * 1024 + 1  # R = 129 groups per thread: masks for 64 + 64 + 1 of them


def _plan_reread():
    """One 64-atom molecule per group, in-degree 3, so no group is on a list but the chosen
    ones: of every three threads of node_group_lists_kernel the first has fallback groups in
    the first, middle and last 64-block of its range, the second in its last block only, the
    third none.  Fallbacks alternate between forward-only (one atom of in-degree cap + 1) and
    both directions (every atom of degree 9: over the edge cap)."""
    K = tier_constants()
    ga, G = K["kNodeGroupAtoms"], PLAN_REREAD_GROUPS
    R = -(-G // 1024)
    deg = np.full((G, ga), 3, np.int64)
    t = np.arange(0, -(-G // R))
    picks = [t[t % 3 == 0] * R + o for o in (0, 5, 63, 64, 100, R - 1)] + [t[t % 3 == 1] * R + R - 1]
    g = np.concatenate(picks + [[G - 1]])
    g = np.unique(g[g < G])
    fwd_only = g[::2]
    both = g[1::2]
    deg[fwd_only, 7] = K["kPlanDegCap"] + 1
    deg[both, :] = K["kPlanEdgeCap"] // ga + 1
    return plan_from(np.full(G, ga), deg.ravel())


_PLAN_CASES = {"caps": _plan_caps, "reread": _plan_reread}
_PLAN_CASES.update({f"G{G}": (lambda G=G: _plan_random(G, G)) for G in (1, 1023, 1024, 1025, 65536, 65537)})
PLAN_CASE_NAMES = tuple(_PLAN_CASES)


@functools.lru_cache(maxsize=2)
def plan_case(name):
    return _PLAN_CASES[name]()


def plan_ref(node_offsets, in_rowptr):
    K = tier_constants()
    return graph_ref.node_group_plan_ref(
        node_offsets, in_rowptr, group_atoms=K["kNodeGroupAtoms"], win_atoms=K["kPlanWinAtoms"],
        edge_cap=K["kPlanEdgeCap"], deg_cap=K["kPlanDegCap"], big_atoms=K["kPlanBigAtoms"],
        big_edge_cap=K["kPlanBigEdgeCap"])


# ------------------------------------------------------------------ driver (GPU)
DEV = "cuda:0"


def build_direct(bnn, bne, src_l, dst_l, device=DEV):
    """mvml_build_csr through the C ABI, allocated as BatchedMolGraph._build_device does, every
    output (the flags too) pre-filled with SENTINEL so that a slot nobody wrote shows.  Returns
    {the eleven index arrays, "status_flags"} as numpy."""
    import torch
    from mvml_gat import _lib
    device = torch.device(device)
    B, N, E = len(bnn), int(np.sum(bnn)), int(np.sum(bne))
    up = lambda a, dt: torch.as_tensor(np.ascontiguousarray(a, dtype=dt)).to(device)
    bnn_d, bne_d = up(bnn, np.int64), up(bne, np.int64)
    src_d, dst_d = up(src_l, np.int32), up(dst_l, np.int32)
    shape = dict(node_offsets=B + 1, edge_offsets=B + 1, src=E, dst=E, node_graph=N,
                 in_rowptr=N + 1, in_src=E, in_eid=E, out_rowptr=N + 1, out_dst=E, out_inslot=E)
    d = {k: torch.full((shape[k],), SENTINEL, device=device,
                       dtype=torch.int64 if k.endswith("offsets") else torch.int32)
         for k in INDEX_KEYS}
    flags = torch.full((2,), SENTINEL, dtype=torch.int32, device=device)
    with torch.cuda.device(device):
        L = _lib.lib()
        wp, wn = _lib.ws_ptr_size(L.mvml_build_csr_workspace_size(B, N, E), device)
        P = _lib.ptr
        _lib.call("mvml_build_csr", P(src_d), P(dst_d), P(bnn_d), P(bne_d), B, N, E,
                  P(d["node_offsets"]), P(d["edge_offsets"]), P(d["src"]), P(d["dst"]),
                  P(d["node_graph"]), P(d["in_rowptr"]), P(d["in_src"]), P(d["in_eid"]),
                  P(d["out_rowptr"]), P(d["out_dst"]), P(d["out_inslot"]), P(flags), wp, wn,
                  _lib.stream_ptr(device))
        torch.cuda.synchronize()
    out = {k: v.cpu().numpy() for k, v in d.items()}
    out["status_flags"] = flags.cpu().numpy()
    return out


def oracle(bnn, bne, src_l, dst_l):
    ref = graph_ref.batch_ref(bnn, src_l, dst_l, bne)
    ref.update(graph_ref.csr_ref(ref["src"], ref["dst"], ref["node_offsets"][-1]))
    return ref


def assert_matches_oracle(out, bnn, bne, src_l, dst_l):
    """All eleven arrays bit-equal to the oracle's; flags[0] is the COUNT of zero-in-degree
    atoms, flags[1] (edges with an id outside their molecule) is 0."""
    ref = oracle(bnn, bne, src_l, dst_l)
    for k in INDEX_KEYS:
        assert out[k].dtype == ref[k].dtype, k
        np.testing.assert_array_equal(out[k], ref[k], err_msg=k)
    assert int(out["status_flags"][0]) == ref["zero_in_degree"]
    assert int(out["status_flags"][1]) == 0
    return ref


def build_plan_direct(node_offsets, in_rowptr, device=DEV):
    """mvml_build_node_groups on host-made inputs; the plan pre-filled with SENTINEL."""
    import torch
    from mvml_gat import _lib
    device = torch.device(device)
    B, N = len(node_offsets) - 1, int(node_offsets[-1])
    no = torch.as_tensor(np.ascontiguousarray(node_offsets, dtype=np.int64)).to(device)
    rp = torch.as_tensor(np.ascontiguousarray(in_rowptr, dtype=np.int32)).to(device)
    with torch.cuda.device(device):
        L = _lib.lib()
        G = int(L.mvml_node_group_count(N))
        plan = torch.full((int(L.mvml_node_group_plan_size(N)),), SENTINEL, dtype=torch.int32,
                          device=device)
        _lib.call("mvml_build_node_groups", B, N, _lib.ptr(no), _lib.ptr(rp), _lib.ptr(plan),
                  _lib.stream_ptr(device))
        torch.cuda.synchronize()
    return G, plan.cpu().numpy()


def assert_plan_matches_oracle(G, plan, node_offsets, in_rowptr):
    starts, kinds, fwd, bwd = plan_ref(node_offsets, in_rowptr)
    assert G == len(kinds) and plan.size == 4 * G + 3
    np.testing.assert_array_equal(plan[:G + 1], starts, err_msg="starts")
    np.testing.assert_array_equal(plan[G + 1:2 * G + 1], kinds, err_msg="kinds")
    assert (int(plan[2 * G + 1]), int(plan[2 * G + 2])) == (len(fwd), len(bwd))
    for name, base, want in (("fwd", 2 * G + 3, fwd), ("bwd", 3 * G + 3, bwd)):
        np.testing.assert_array_equal(plan[base:base + len(want)], sorted(want), err_msg=name)
        assert np.all(plan[base + len(want):base + G] == SENTINEL), name + " list tail written"
