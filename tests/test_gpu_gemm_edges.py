"""The GEMM paths (csrc/gemm_f32.hip, gemm_smallk.hip, gemm_prep.hip, gemm_common.h) at every tile
edge, layout, alignment and epilogue against a float64 reference, element by element
(_gemm_cases.py: the tables, the two kinds of input, the bars).

Every operand is a view into a larger device buffer of NaN poison (a margin before and after, the
pitch gaps, the rows after row K - 1 of a K-major operand), at an offset inside it.  After a call
 * everything of C's buffer outside [M][N] is bitwise the poison;
 * C inside is finite (with beta == 0 it was poison before): a NaN means a gap value reached the
   arithmetic, be it through a multiply by zero;
 * kind (a), exact inputs: C equals the float64 result cast to fp32 (torch.equal), whatever the
   precision, tile, layout or summation order — a missing, doubled or stale k, a wrong row scale
   or a clamped neighbour's element is an integer-sized difference;
 * kind (b), real inputs: |C - ref| <= (3 * 2^-22 + 4 e_cpu) den element-wise (+ 2^-21 |ref| with
   the ELU / ELU' epilogues), e_cpu from torch's CPU fp32 product of the same inputs.  e, e_cpu
   and the bar of every case go to parity_margins/gemm_edges.json.
The il4 images are made by mvml_split_f16x2_il4 from the poisoned fp32 operand into zeroed memory.
Some 1,400 products of at most 800 x 800 x 2100, twice; the file runs in about 7 s on an MI355X.

Out of scope here: the LSTM-cell epilogue entries (pinned by the Set2Set and SMILES shape tests),
mvml_gemm_f16x2_planes (not called by the model; test_gpu_planes.py) and the timing ablations.
"""
import contextlib
import ctypes
import json
import os

import pytest
import torch

import _gemm_cases as G
from _placed import Placed
from mvml_gat._lib import MvmlError, call, lib, option, stream_ptr, ws_ptr_size

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GROUPS = G.groups()
MARGINS = {}


def _p(t):
    return None if t is None else t.ptr()


def _launch(c, inp, st):
    """Place the operands of a case, run its entry point, return (C, extras)."""
    L = lib()
    z, M, N, K = c.batch, c.M, c.N, c.K
    gap = 8 if z > 1 else 0
    A = Placed((z, K, M) if c.ak else (z, M, K), c.lda, c.off_a, gap, 2 if c.ak else 0,
               inp["A"].transpose(1, 2) if c.ak else inp["A"])
    B = Placed((z, K, N) if c.bk else (z, N, K), c.ldb, 0, gap, 2 if c.bk else 0,
               inp["B"].transpose(1, 2) if c.bk else inp["B"])
    C = Placed((z, M, N), c.ldc, c.off_c, 2 * gap, 0, inp["C0"])
    bias = None
    if inp["bias"] is not None:
        bias = Placed((inp["bias"].shape[0], 1, N), N, c.off_bias, 5 if z > 1 else 0, 0, inp["bias"])
    mx = torch.zeros(2, dtype=torch.int32, device=DEV)
    sl = [ctypes.c_void_p(mx.data_ptr()), ctypes.c_void_p(mx.data_ptr() + 4)]
    for zi in range(z):   # the maxima of exactly the elements the products read
        call("mvml_absmax_f32", A.rows, A.cols, A.ptr(zi), A.ld, sl[0], int(zi > 0), st)
        call("mvml_absmax_f32", B.rows, B.cols, B.ptr(zi), B.ld, sl[1], int(zi > 0), st)
    img = None
    if c.il4 or c.entry == "f16x2_bsplit":
        img = Placed((z, B.rows, B.cols), B.ld, 0, gap, 2 if c.bk else 0)
        img.buf.zero_()
        for zi in range(z):
            call("mvml_split_f16x2_il4", B.rows, B.cols, B.ptr(zi), B.ld, sl[1], img.ptr(zi), st)
    rows = None
    if c.entry in ("f16x2_rows", "f16x2_ex"):
        rows = Placed((z, 1, M), M, 0, 3 if z > 1 else 0)
        for zi in range(z):
            call("mvml_absmax_rows_f32", M, K, A.ptr(zi), A.ld, rows.ptr(zi), 0, st)
    if c.splitk:
        assert L.mvml_gemm_workspace_size(M, N, K) > 256, "no split-K slab"
    wp, wn = ws_ptr_size(L.mvml_gemm_workspace_size(M, N, K), DEV)
    ex = {}
    e = c.entry
    if e in ("f32", "f32x3", "bf16", "f16x2"):
        call("mvml_gemm_" + e, c.ak, c.bk, M, N, K, A.ptr(), A.ld, B.ptr(), B.ld, _p(bias), c.beta, c.act,
             C.ptr(), C.ld, wp, wn, st)
    elif e == "f16x2_amax":
        call("mvml_gemm_f16x2_amax", c.ak, c.bk, M, N, K, A.ptr(), A.ld, B.ptr(), B.ld, sl[0], sl[1], _p(bias),
             c.beta, c.act, C.ptr(), C.ld, wp, wn, st)
    elif e == "f16x2_bsplit":
        call("mvml_gemm_f16x2_bsplit", c.ak, c.bk, M, N, K, A.ptr(), A.ld, B.ptr(), B.ld, img.ptr(), 0, sl[0],
             sl[1], _p(bias), c.beta, c.act, C.ptr(), C.ld, wp, wn, st)
    elif e == "f16x2_rows":
        if c.smallk >= 0:
            sk = L.mvml_gemm_rows_smallk(c.bk, M, N, K, A.ptr(), A.ld, (img or B).ptr(), B.ld, c.beta, c.act,
                                         C.ptr(), C.ld)
            assert sk == c.smallk, f"mvml_gemm_rows_smallk = {sk}, expected {c.smallk}"
        call("mvml_gemm_f16x2_rows", M, N, K, A.ptr(), A.ld, B.ptr(), B.ld, c.bk, _p(img), rows.ptr(), sl[1],
             _p(bias), c.beta, c.act, C.ptr(), C.ld, wp, wn, st)
    elif e == "f16x2_ex":
        slots = 1 if c.rows_cols == 0 else -(-N // c.rows_cols)
        crows = Placed((z, slots, M), M + 3, 1, 7 if z > 1 else 0, 0, torch.zeros(z, slots, M))
        camax = torch.zeros(1, dtype=torch.int32, device=DEV)
        aux = None
        if c.act == 3:
            aux = Placed((1, M, N), N + c.pad_aux, 0, 0, 0, inp["aux"])
        call("mvml_gemm_f16x2_ex", M, N, K, z, A.ptr(), A.ld, A.stride, B.ptr(), B.ld, c.bk, _p(img), B.stride,
             rows.ptr(), rows.stride, sl[1], _p(bias), bias.stride if bias else 0, c.act, C.ptr(), C.ld,
             C.stride, _p(aux), aux.ld if aux else 0, ctypes.c_void_p(camax.data_ptr()), crows.ptr(),
             crows.ld, c.rows_cols, crows.stride, st)
        ex = {"crows": crows, "camax": camax, "slots": slots}
    elif e == "f16x2_batched":
        call("mvml_gemm_f16x2_batched", c.ak, c.bk, M, N, K, z, A.ptr(), A.ld, A.stride, B.ptr(), B.ld, B.stride,
             sl[0], sl[1], C.ptr(), C.ld, C.stride, st)
    elif e == "f32x3_batched":
        call("mvml_gemm_f32x3_batched", c.ak, c.bk, M, N, K, z, A.ptr(), A.ld, A.stride, B.ptr(), B.ld, B.stride,
             _p(bias), c.beta, c.act, C.ptr(), C.ld, C.stride, st)
    elif e == "colsum":
        fused = L.mvml_gemm_colsum_fused(M, N, K)
        assert fused == c.fused, f"mvml_gemm_colsum_fused = {fused}, expected {c.fused}"
        sums = Placed((1, 1, c.sum_n), c.sum_n, 1)
        wp, wn = ws_ptr_size(L.mvml_gemm_colsum_workspace_size(M, N, K, c.sum_n), DEV)
        call("mvml_gemm_f16x2_amax_colsum", M, N, K, A.ptr(), A.ld, B.ptr(), B.ld, sl[0], sl[1], C.ptr(), C.ld,
             c.sum_off, c.sum_n, c.alpha, sums.ptr(), wp, wn, st)
        ex = {"sums": sums}
    else:
        raise AssertionError(e)
    torch.cuda.synchronize()
    return C, ex


def _where(count, idx):
    return f"{count} elements, first at (batch, row, col) = {idx}"


def _check(c, kind, inp, C, ex):
    """Every failed property of one run as a string."""
    errs = []
    ref, pre, den = G.reference(c, inp)
    n, pos = C.outside()
    if n:
        errs.append(f"C's buffer outside [M][N] overwritten: {_where(n, pos)}")
    got = C.read()
    nf = ~torch.isfinite(got)
    if bool(nf.any()):
        errs.append(f"non-finite C: {_where(int(nf.sum()), tuple(nf.nonzero()[0].tolist()))}")
    rec = {"entry": c.entry, "kind": kind}
    if kind == "a":
        want = ref.float()
        if c.act == 2:   # ELU of a negative value is not exact: 4 ulp there, equality elsewhere
            neg = pre < 0
            tol_bad = neg & ((got.double() - ref).abs() > G.ELU_ULP * ref.abs())
            ne = (~neg & (got != want)) | tol_bad
            cnt, idx = int(ne.sum()), (tuple(ne.nonzero()[0].tolist()) if bool(ne.any()) else None)
        else:
            cnt, idx = G.first_diff(got, want)
            assert (cnt == 0) == torch.equal(got, want)
        if cnt:
            errs.append(f"C != float64 reference: {_where(cnt, idx)}: got {got[idx].item()!r}, "
                        f"reference {want[idx].item()!r}")
    else:
        e_cpu = G.stat(G.cpu_fp32_pre(c, inp), pre, den)
        b = G.bar(e_cpu)
        slack = G.ELU_ULP * ref.abs() if c.act >= 2 else torch.zeros_like(ref)
        excess = ((got.double() - ref).abs() - slack).clamp_min(0.0)
        e = G.stat(ref + excess, ref, den)
        rec.update(e=e, e_cpu=e_cpu, bar=b)
        if not e <= b:
            r = torch.nan_to_num(excess / den.clamp_min(1e-300), nan=float("inf"))
            idx = tuple((r == r.max()).nonzero()[0].tolist())
            errs.append(f"e = {e:.3e} > bar {b:.3e} (e_cpu {e_cpu:.3e}), worst at (batch, row, col) = {idx}: "
                        f"got {got[idx].item()!r}, reference {ref[idx].item()!r}")
    if "crows" in ex:
        bits = got.abs().contiguous().view(torch.int32)
        w = c.rows_cols or c.N
        want_rows = torch.stack([bits[:, :, s * w:(s + 1) * w].amax(2) for s in range(ex["slots"])], 1)
        have = ex["crows"].read(torch.int32)
        if not torch.equal(have, want_rows):
            cnt, idx = G.first_diff(have, want_rows)
            errs.append(f"c_rows != row maxima of the returned C: {cnt} entries, first (batch, slot, row) = {idx}")
        n, pos = ex["crows"].outside()
        if n:
            errs.append(f"c_rows written outside its slots: {_where(n, pos)}")
        if int(ex["camax"].item()) != int(bits.max()):
            errs.append(f"c_amax bits {int(ex['camax'].item()):#x} != max |C| bits {int(bits.max()):#x}")
    if "sums" in ex:
        s_ref, s_abs = G.colsum_reference(c, inp)
        s = ex["sums"].read()[0, 0]
        n, pos = ex["sums"].outside()
        if n:
            errs.append(f"sum_out written outside [sum_n]: {_where(n, pos)}")
        if kind == "a":
            if not torch.equal(s, s_ref.float()):
                cnt, idx = G.first_diff(s, s_ref.float())
                errs.append(f"column sums != float64: {cnt} columns, first {idx}")
        else:
            rows = inp["A"][0, c.sum_off:c.sum_off + c.sum_n]
            es_cpu = G.stat(c.alpha * rows.sum(1), s_ref, s_abs)
            es = G.stat(s, s_ref, s_abs)
            bs = 2.0 ** -22 + 4.0 * es_cpu
            rec.update(e_sum=es, e_sum_cpu=es_cpu, bar_sum=bs)
            if not es <= bs:
                errs.append(f"column sums: e = {es:.3e} > bar {bs:.3e} (CPU fp32 {es_cpu:.3e})")
    if kind == "b":
        MARGINS[c.name] = rec
    return errs


def run_case(c, kind):
    inp = G.make_inputs(c, kind)
    with contextlib.ExitStack() as stack:
        for name, value in c.opts:
            stack.enter_context(option(name, value))
        try:
            C, ex = _launch(c, inp, stream_ptr())
        except (MvmlError, AssertionError) as err:   # a refused call or a wrong plan: no device fault
            return [f"{type(err).__name__}: {err}"]
        except RuntimeError as err:   # a device error: launch nothing more on this GPU
            pytest.exit(f"device error in {c.name}: {err}", returncode=3)
    return _check(c, kind, inp, C, ex)


@pytest.fixture(scope="module", autouse=True)
def _margins_file():
    yield
    out = os.environ.get("MVML_MARGINS_DIR", os.path.join(os.path.dirname(os.path.dirname(
        os.path.abspath(__file__))), "parity_margins"))
    os.makedirs(out, exist_ok=True)
    worst = {}
    for rec in MARGINS.values():
        worst[rec["entry"]] = max(worst.get(rec["entry"], 0.0), rec["e"] / rec["bar"])
    with open(os.path.join(out, "gemm_edges.json"), "w") as f:
        json.dump({"worst_e_over_bar": worst, "cases": MARGINS}, f, indent=1)
    print("worst e / bar per entry:", {k: round(v, 3) for k, v in sorted(worst.items())})


@pytest.mark.parametrize("kind", ["a", "b"])
@pytest.mark.parametrize("group", sorted(GROUPS))
def test_gemm_edges(group, kind):
    """Every case of one (table, entry, layout) with exact (a) or real (b) inputs; all failures of
    the group are reported together, each with its case and first wrong element."""
    cases = [c for c in GROUPS[group] if kind in c.kind_list()]
    if not cases:
        assert kind == "b"   # the plain-bf16 entry and the persistent-loop table: kind (a) only
        return
    fails = []
    for c in cases:
        fails += [f"{c.name} [{', '.join(c.labels)}]: {msg}" for msg in run_case(c, kind)]
    assert not fails, f"{len(fails)} failures in {len(cases)} cases:\n" + "\n".join(fails[:40])
