"""The parameter side of a GAT layer at the ABI (csrc/gat_params.hip, the projection's logit-partial
epilogue of csrc/gemm_f32.hip) against float64, element by element (_gat_param_cases.py: the
tables, the two kinds of input, the bars; _placed.py: the poisoned buffers).

Every input and output is a view into a larger device buffer of NaN poison (a margin before and
after, pitches wider than the rows).  After a call
 * every word outside the documented output region is bitwise the poison (Y's columns past C, Wcat's
   last 2H rows without attn_lr, g_res_fc_w under MVML_RES_NONE, rows past the row count) and Wcat's
   pad columns are +0.0;
 * everything inside is finite: poison in a region the kernel must not read (gW's pad columns, X's
   pitch gap, Y's columns past H F, gelr's past 2H) would show as a NaN;
 * kind (a), exact inputs: the result equals the float64 result cast to fp32 (torch.equal);
 * kind (b), real inputs: |x - ref| <= bar * den element-wise, the bar derived per kernel.  e, the
   bar and e / bar of every case go to parity_margins/gat_params.json (MVML_MARGINS_DIR).
Every projection case forces gemm_tile, so its kernel instance is the case's label; the table
reaches all 32 instances with the epilogue (test_gat_param_cases_cpu.py).  Every documented
refusal returns its code, names its entry in mvml_last_error() and leaves the outputs poison.
About 1,100 small calls; the file runs in some seconds on an MI355X.
"""
import contextlib
import ctypes
import json
import os
import time

import pytest
import torch

import _gat_param_cases as P
import _gemm_cases as G
from _placed import DEV, Placed
from mvml_gat._lib import MvmlError, call, lib, option, stream_ptr

pytestmark = pytest.mark.gpu
PROJ_GROUPS = P.proj_groups()
MARGINS = {}
INVALID, WORKSPACE = 1, 3     # MVML_ERR_*


def _p(t):
    return None if t is None else t.ptr()


def _where(count, idx):
    return f"{count} elements, first at (batch, row, col) = {idx}"


def _bits(t):
    return t.contiguous().view(torch.int32)


def _untouched(name, pl, errs):
    """The whole buffer of a Placed (its matrix included) is still poison."""
    n = int((pl.buf.view(torch.int32) != G.POISON_BITS).sum())
    if n:
        errs.append(f"{name}: {n} words written where nothing may be")


def _outside(name, pl, errs):
    n, pos = pl.outside()
    if n:
        errs.append(f"{name}: written outside its region: {_where(n, pos)}")


def _finite(name, got, errs):
    nf = ~torch.isfinite(got)
    if bool(nf.any()):
        errs.append(f"{name}: non-finite: {_where(int(nf.sum()), tuple(nf.nonzero()[0].tolist()))}")


def _exact(name, got, ref64, errs):
    want = ref64.float()
    cnt, idx = G.first_diff(got, want)
    assert (cnt == 0) == torch.equal(got, want)
    if cnt:
        errs.append(f"{name} != float64 reference: {_where(cnt, idx)}: got {got[idx].item()!r}, "
                    f"reference {want[idx].item()!r}")


def _bitwise(name, got, want, errs):
    cnt, idx = G.first_diff(_bits(got), _bits(want))
    if cnt:
        errs.append(f"{name}: not bitwise equal: {_where(cnt, idx)}")


def _held(name, case, kernel, got, ref, den, bar, errs):
    """Kind (b): e = max |got - ref| / den against the bar; recorded for gat_params.json."""
    e = G.stat(got, ref, den)
    MARGINS[f"{case}:{name}"] = {"kernel": kernel, "e": e, "bar": bar, "ratio": e / bar}
    if not e <= bar:
        r = torch.nan_to_num((got.double() - ref).abs() / den.clamp_min(1e-300), nan=float("inf"))
        idx = tuple((r == r.max()).nonzero()[0].tolist())
        errs.append(f"{name}: e = {e:.3e} > bar {bar:.3e}, worst at {idx}: got {got[idx].item()!r}, "
                    f"reference {ref[idx].item()!r}")


def _guard(fn, name):
    """Run the launches of one case: a refused call is a failure of the case, a device error ends
    the session (nothing more is launched on this GPU)."""
    try:
        return fn(), []
    except (MvmlError, AssertionError) as err:
        return None, [f"{type(err).__name__}: {err}"]
    except RuntimeError as err:
        pytest.exit(f"device error in {name}: {err}", returncode=3)


def _report(fails, n):
    assert not fails, f"{len(fails)} failures in {n} cases:\n" + "\n".join(fails[:40])


@pytest.fixture(scope="module", autouse=True)
def _margins_file():
    t0 = time.time()
    yield
    torch.cuda.synchronize()
    out = os.environ.get("MVML_MARGINS_DIR", os.path.join(os.path.dirname(os.path.dirname(
        os.path.abspath(__file__))), "parity_margins"))
    os.makedirs(out, exist_ok=True)
    worst = {}
    for rec in MARGINS.values():
        worst[rec["kernel"]] = max(worst.get(rec["kernel"], 0.0), rec["ratio"])
    with open(os.path.join(out, "gat_params.json"), "w") as f:
        json.dump({"worst_e_over_bar": worst, "seconds": time.time() - t0, "cases": MARGINS}, f, indent=1)
    print("worst e / bar per kernel:", {k: round(v, 3) for k, v in sorted(worst.items())})
    print(f"test_gpu_gat_params.py: {time.time() - t0:.1f} s")


# ====================================================================== 1. mvml_gat_proj_fwd
def _absmax(pl, rows, cols, slot):
    call("mvml_absmax_f32", rows, cols, pl.ptr(), pl.ld, ctypes.c_void_p(slot), 0, stream_ptr())


def _proj_launch(c, inp, maxima=None):
    """Place a projection case and run it: (Y, elr, workspace) as Placed."""
    L = lib()
    assert L.mvml_gat_proj_cols_res(c.H, c.F, c.res) == c.C
    if c.res != P.RES_NONE:
        assert L.mvml_gat_proj_cols(c.H, c.F, c.res) == c.C
    X = Placed((1, c.N, c.K), c.ldx, c.off_x, 0, 1, inp["X"])
    W = Placed((1, c.C, c.K), c.ldw, 0, 0, 1, inp["W"])
    a = Placed((1, 2, c.HF), c.HF, 0, 0, 0, inp["a"])
    Y = Placed((1, c.N, c.C), c.C + 4, 0, 0, 2)
    elr = Placed((1, c.N, 2 * c.H), 2 * c.H, 0, 0, 1)
    wsz = L.mvml_gat_proj_fwd_workspace_size(c.N, c.H, c.F)
    assert wsz % 4 == 0
    ws = Placed((1, 1, wsz // 4), wsz // 4)
    mx = torch.zeros(2, dtype=torch.int32, device=DEV)
    px = pw = None
    maxima = maxima or c.maxima
    if c.algo == "f16x2" and c.wide and maxima != "null":   # over exactly the elements read
        _absmax(X, c.N, c.K, mx.data_ptr())
        px = ctypes.c_void_p(mx.data_ptr())
        if maxima == "given":
            _absmax(W, c.C, c.K, mx.data_ptr() + 4)
            pw = ctypes.c_void_p(mx.data_ptr() + 4)
    with contextlib.ExitStack() as stack:
        stack.enter_context(option("gemm_tile", c.tile))
        if c.persist >= 0:
            stack.enter_context(option("gemm_persist", c.persist))
        call("mvml_gat_proj_fwd", c.N, X.ptr(), X.ld, c.K, W.ptr(), W.ld, a.ptr(), c.H, c.F, c.res, P.ALGO[c.algo],
             Y.ptr(), Y.ld, elr.ptr(), px, pw, None, 0, ws.ptr(), wsz, stream_ptr())
    torch.cuda.synchronize()
    return Y, elr, ws


def _proj_check(c, kind, inp, Y, elr, ws):
    errs = []
    _outside("Y", Y, errs)
    _outside("elr", elr, errs)
    _outside("workspace", ws, errs)
    y, el = Y.read()[0], elr.read()[0]
    _finite("Y", y, errs)
    _finite("elr", el, errs)
    Y64, el64, den_y, den_el = P.proj_reference(c, inp)
    if kind == "a":
        _exact("Y", y, Y64, errs)
        _exact("elr", el, el64, errs)
    else:
        y32, el32 = P.proj_cpu_fp32(c, inp)
        kern = c.labels[0].rsplit("-lw", 1)[0]
        _held("Y", c.name, f"proj_fwd Y {kern}", y, Y64, den_y, G.bar(G.stat(y32, Y64, den_y)), errs)
        _held("elr", c.name, f"proj_fwd elr {kern}", el, el64, den_el, G.bar(G.stat(el32, el64, den_el)), errs)
    return errs


@pytest.mark.parametrize("kind", ["a", "b"])
@pytest.mark.parametrize("group", sorted(PROJ_GROUPS))
def test_proj_fwd(group, kind):
    """Every case of one (algo, forced tile): Y[:, :C] and [el | er] element-wise."""
    cases = [c for c in PROJ_GROUPS[group] if kind in c.kinds()]
    if not cases:
        assert kind == "b" and group.startswith("bf16")   # plain bf16 operands: kind (a) only
        return
    fails = []
    for c in cases:
        inp = P.proj_inputs(c, kind)
        res, errs = _guard(lambda: _proj_launch(c, inp), c.name)
        if res is not None:
            errs = _proj_check(c, kind, inp, *res)
        fails += [f"{c.name} [{', '.join(c.labels)}]: {m}" for m in errs]
    _report(fails, len(cases))


@pytest.mark.parametrize("kind", ["a", "b"])
def test_proj_fwd_maxima_variants(kind):
    """MVML_GEMM_F16X2 on the 256x256 kernel: maxima supplied, both NULL, or only one supplied (then
    the entry computes them in its workspace) give bitwise the same Y and elr, fast and guarded."""
    fails = []
    by_shape = {}
    for c in P.PROJ_MAXIMA:
        by_shape.setdefault((c.K, c.pad_x), []).append(c)
    for cases in by_shape.values():
        base = cases[0]
        inp = P.proj_inputs(base, kind)
        outs = {}
        for c in cases:
            res, errs = _guard(lambda: _proj_launch(base, inp, c.maxima), c.name)
            if res is not None:
                errs = _proj_check(base, kind, inp, *res) if c.maxima == "given" else []
                outs[c.maxima] = (res[0].read(), res[1].read())
            fails += [f"{c.name}: {m}" for m in errs]
        for m in ("null", "one"):
            if m in outs and "given" in outs:
                _bitwise(f"{base.name} Y, maxima {m} vs given", outs[m][0], outs["given"][0], fails)
                _bitwise(f"{base.name} elr, maxima {m} vs given", outs[m][1], outs["given"][1], fails)
    _report(fails, len(P.PROJ_MAXIMA))


@pytest.mark.parametrize("algo", list(P.ALGO))
def test_proj_fwd_no_rows(algo):
    """num_nodes = 0: MVML_OK, nothing written, a NULL workspace accepted."""
    c = P.Proj(algo, 256, 0, 76, 2, 24, P.RES_MEAN)
    inp = P.proj_inputs(P.Proj(algo, 256, 4, 76, 2, 24, P.RES_MEAN), "b")
    W = Placed((1, c.C, c.K), c.ldw, 0, 0, 1, inp["W"])
    a = Placed((1, 2, c.HF), c.HF, 0, 0, 0, inp["a"])
    X, Y, elr = Placed((1, 1, c.K), c.K), Placed((1, 1, c.C), c.C + 4), Placed((1, 1, 2 * c.H), 2 * c.H)
    assert lib().mvml_gat_proj_fwd_workspace_size(0, c.H, c.F) >= 256
    call("mvml_gat_proj_fwd", 0, X.ptr(), c.K, c.K, W.ptr(), W.ld, a.ptr(), c.H, c.F, c.res, P.ALGO[algo], Y.ptr(),
         Y.ld, elr.ptr(), None, None, None, 0, None, 0, stream_ptr())
    torch.cuda.synchronize()
    errs = []
    _untouched("Y", Y, errs)
    _untouched("elr", elr, errs)
    assert not errs, errs


def _refused(entry, who, code, outputs, *args):
    """A refused call: its code, the entry named in mvml_last_error(), the outputs still poison."""
    L = lib()
    rc = getattr(L, entry)(*args)
    msg = L.mvml_last_error().decode(errors="replace")
    torch.cuda.synchronize()
    errs = []
    if rc != code:
        errs.append(f"returned {rc}, expected {code} ({msg!r})")
    if who not in msg:
        errs.append(f"mvml_last_error() = {msg!r} does not name {who}")
    for name, pl in outputs.items():
        _untouched(name, pl, errs)
    return errs


PROJ_REFUSALS = {
    "H=3": (dict(H=3), INVALID), "F=6": (dict(F=6), INVALID), "K=0": (dict(K=0), INVALID),
    "ldx<K": (dict(ldx=7), INVALID), "ldw<K": (dict(ldw=7), INVALID), "ldy<C": (dict(ldy=15), INVALID),
    "algo": (dict(algo=7), INVALID), "w_planes": (dict(w_planes=True), INVALID),
    "attn_lr NULL": (dict(attn=False), INVALID), "elr NULL": (dict(elr=False), INVALID),
    "workspace short": (dict(ws_short=1), WORKSPACE), "workspace NULL": (dict(ws=False), WORKSPACE),
}


@pytest.mark.parametrize("what", list(PROJ_REFUSALS))
def test_proj_fwd_refusals(what):
    kw, code = PROJ_REFUSALS[what]
    N, K, H, F = 5, 8, 2, 4              # C = 16 with a projected residual
    X, W = Placed((1, N, K), K, data=torch.ones(N, K)), Placed((1, 16 + 2 * H, K), K, data=torch.ones(20, K))
    a = Placed((1, 2, 8), 8, data=torch.ones(2, 8))
    Y, elr = Placed((1, N, 16), 16), Placed((1, N, 2 * H), 2 * H)
    wsz = lib().mvml_gat_proj_fwd_workspace_size(N, H, F)
    ws = Placed((1, 1, wsz // 4), wsz // 4)
    planes = Placed((1, 1, 64), 64)
    errs = _refused(
        "mvml_gat_proj_fwd", "gat_proj_fwd", code, {"Y": Y, "elr": elr, "workspace": ws},
        N, X.ptr(), kw.get("ldx", K), kw.get("K", K), W.ptr(), kw.get("ldw", K), a.ptr() if kw.get("attn", True) else None,
        kw.get("H", H), kw.get("F", F), P.RES_PROJ, kw.get("algo", 0), Y.ptr(), kw.get("ldy", 16),
        elr.ptr() if kw.get("elr", True) else None, None, None, planes.ptr() if kw.get("w_planes") else None, 0,
        ws.ptr() if kw.get("ws", True) else None, wsz - kw.get("ws_short", 0), stream_ptr())
    assert not errs, errs


# ====================================================================== 2. fold_weights
def _fold_run(c, inp, res_entry):
    fc = Placed((1, c.HF, c.Fin), c.Fin, data=inp["fc"])
    res = Placed((1, c.HF, c.Fin), c.Fin, data=inp["res"]) if c.res != P.RES_NONE else None
    a = Placed((1, 2, c.HF), c.HF, data=inp["a"]) if c.attn else None
    Wc = Placed((1, c.rows, c.ld), c.ld, 0, 0, 2 * c.H + 1)
    if res_entry:
        call("mvml_gat_fold_weights_res", fc.ptr(), _p(res), _p(a), c.H, c.F, c.Fin, c.ld, c.res, Wc.ptr(), stream_ptr())
    else:
        call("mvml_gat_fold_weights", fc.ptr(), _p(res), _p(a), c.H, c.F, c.Fin, c.ld, int(c.res == P.RES_MEAN),
             Wc.ptr(), stream_ptr())
    torch.cuda.synchronize()
    return Wc


def _fold_check(c, kind, inp, Wc):
    errs = []
    _outside("Wcat", Wc, errs)      # (without attn_lr: the 2H rows after the projection rows too)
    full = Wc.read()[0]
    got, pad = full[:, :c.Fin], full[:, c.Fin:]
    _finite("Wcat", full, errs)
    if bool((_bits(pad) != 0).any()):
        errs.append(f"Wcat's pad columns are not +0.0: {int((_bits(pad) != 0).sum())} words")
    ref, den = P.fold_reference(c, inp["fc"], inp["res"], inp["a"])
    _bitwise("fc rows", got[:c.HF], inp["fc"], errs)
    if c.res == P.RES_PROJ:
        _bitwise("res_fc rows", got[c.HF:c.C], inp["res"], errs)
    if kind == "a":
        _exact("Wcat", got, ref, errs)
    else:
        if c.res == P.RES_MEAN:
            _held("mean rows", c.name, "fold_weights mean rows", got[c.HF:c.C], ref[c.HF:c.C], den[c.HF:c.C],
                  c.H * P.U, errs)
        if c.attn:
            _held("A rows", c.name, "fold_weights A rows", got[c.C:], ref[c.C:], den[c.C:], c.F * P.U, errs)
    return errs


@pytest.mark.parametrize("kind", ["a", "b"])
@pytest.mark.parametrize("hf", P.FOLD_HF, ids=lambda hf: "h%df%d" % hf)
def test_fold_weights(hf, kind):
    cases = [c for c in P.FOLD_CASES if (c.H, c.F) == hf]
    fails = []
    for c in cases:
        inp = P.fold_inputs(c, kind)
        Wc, errs = _guard(lambda: _fold_run(c, inp, True), c.name)
        if Wc is not None:
            errs = _fold_check(c, kind, inp, Wc)
            if c.res != P.RES_NONE:   # the entry without _res: bitwise the same rows
                W2, errs2 = _guard(lambda: _fold_run(c, inp, False), c.name)
                errs += errs2
                if W2 is not None:
                    _bitwise("mvml_gat_fold_weights vs _res", W2.buf, Wc.buf, errs)
        fails += [f"{c.name}: {m}" for m in errs]
    _report(fails, len(cases))


def test_fold_weights_second_pass():
    assert any(c.rows * c.ld > P.FOLD_GRID_CAP for c in P.FOLD_CASES)


@pytest.mark.parametrize("entry,what", [(e, w) for e in ("mvml_gat_fold_weights_res", "mvml_gat_fold_weights")
                                        for w in ("H=0", "F=0", "Fin=0", "ldw<Fin", "res=3", "res_fc_w NULL PROJ",
                                                  "res_fc_w NULL MEAN")
                                        # (without _res, mean_residual is a flag: any nonzero value is MEAN)
                                        if not (w == "res=3" and not e.endswith("_res"))])
def test_fold_weights_refusals(entry, what):
    H, F, Fin, ld, res = 2, 4, 6, 8, P.RES_PROJ
    fc, rs = Placed((1, 8, 6), 6, data=torch.ones(8, 6)), Placed((1, 8, 6), 6, data=torch.ones(8, 6))
    a, Wc = Placed((1, 2, 8), 8, data=torch.ones(2, 8)), Placed((1, 20, 8), 8)
    rp = rs.ptr()
    if what == "H=0":
        H = 0
    elif what == "F=0":
        F = 0
    elif what == "Fin=0":
        Fin = 0
    elif what == "ldw<Fin":
        ld = 5
    elif what == "res=3":
        res = 3
    else:
        rp, res = None, (P.RES_MEAN if what.endswith("MEAN") else P.RES_PROJ)
    errs = _refused(entry, "gat_fold_weights", INVALID, {"Wcat": Wc}, fc.ptr(), rp, a.ptr(), H, F, Fin, ld, res,
                    Wc.ptr(), stream_ptr())
    assert not errs, errs


# ====================================================================== 3. unfold_grads
def _unfold_run(c, inp, res_entry):
    gW = Placed((1, c.rows, c.Fin), c.ld, 0, 0, 1, inp["gW"])
    a = Placed((1, 2, c.HF), c.HF, data=inp["a"]) if c.attn else None
    g_fc = Placed((1, c.HF, c.Fin), c.Fin)
    # MVML_RES_NONE: g_res_fc_w is not written (with attn_lr: a buffer that must stay poison;
    # without: NULL is accepted)
    g_res = Placed((1, c.HF, c.Fin), c.Fin) if (c.res != P.RES_NONE or c.attn) else None
    if res_entry:
        call("mvml_gat_unfold_grads_res", gW.ptr(), _p(a), c.H, c.F, c.Fin, c.ld, c.res, g_fc.ptr(), _p(g_res),
             stream_ptr())
    else:
        call("mvml_gat_unfold_grads", gW.ptr(), _p(a), c.H, c.F, c.Fin, c.ld, int(c.res == P.RES_MEAN), g_fc.ptr(),
             _p(g_res), stream_ptr())
    torch.cuda.synchronize()
    return g_fc, g_res


def _unfold_check(c, kind, inp, g_fc, g_res):
    errs = []
    _outside("g_fc_w", g_fc, errs)
    got = g_fc.read()[0]
    _finite("g_fc_w", got, errs)
    r_fc, r_res, den = P.unfold_reference(c, inp["gW"], inp["a"])
    if kind == "a":
        _exact("g_fc_w", got, r_fc, errs)
    else:
        _held("g_fc_w", c.name, "unfold_grads g_fc", got, r_fc, den, 2 * P.U, errs)
    if c.res == P.RES_NONE:
        if g_res is not None:
            _untouched("g_res_fc_w under MVML_RES_NONE", g_res, errs)
        return errs
    _outside("g_res_fc_w", g_res, errs)
    gr = g_res.read()[0]
    _finite("g_res_fc_w", gr, errs)
    if kind == "a" or c.res == P.RES_PROJ or P.pow2(c.H):
        _exact("g_res_fc_w", gr, r_res, errs)             # copies, or an exact division: bitwise
        if c.res == P.RES_PROJ:
            _bitwise("g_res_fc_w", gr, inp["gW"][c.HF:2 * c.HF], errs)
    else:
        _held("g_res_fc_w", c.name, "unfold_grads g_res (H = 3)", gr, r_res, r_res.abs(), P.U, errs)
    return errs


@pytest.mark.parametrize("kind", ["a", "b"])
@pytest.mark.parametrize("hf", P.FOLD_HF, ids=lambda hf: "h%df%d" % hf)
def test_unfold_grads(hf, kind):
    cases = [c for c in P.FOLD_CASES if (c.H, c.F) == hf]
    fails = []
    for c in cases:
        inp = P.unfold_inputs(c, kind)
        res, errs = _guard(lambda: _unfold_run(c, inp, True), c.name)
        if res is not None:
            errs = _unfold_check(c, kind, inp, *res)
            if c.res != P.RES_NONE:
                r2, errs2 = _guard(lambda: _unfold_run(c, inp, False), c.name)
                errs += errs2
                if r2 is not None:
                    _bitwise("mvml_gat_unfold_grads g_fc vs _res", r2[0].buf, res[0].buf, errs)
                    _bitwise("mvml_gat_unfold_grads g_res vs _res", r2[1].buf, res[1].buf, errs)
        fails += [f"{c.name}: {m}" for m in errs]
    _report(fails, len(cases))


@pytest.mark.parametrize("entry,what", [(e, w) for e in ("mvml_gat_unfold_grads_res", "mvml_gat_unfold_grads")
                                        for w in ("H=0", "F=0", "Fin=0", "ldg<Fin", "res=3", "g_res_fc_w NULL PROJ",
                                                  "g_res_fc_w NULL MEAN")
                                        # (without _res, mean_residual is a flag: any nonzero value is MEAN)
                                        if not (w == "res=3" and not e.endswith("_res"))])
def test_unfold_grads_refusals(entry, what):
    H, F, Fin, ld, res = 2, 4, 6, 8, P.RES_PROJ
    gW, a = Placed((1, 20, 6), 8, data=torch.ones(20, 6)), Placed((1, 2, 8), 8, data=torch.ones(2, 8))
    g_fc, g_res = Placed((1, 8, 6), 6), Placed((1, 8, 6), 6)
    rp = g_res.ptr()
    if what == "H=0":
        H = 0
    elif what == "F=0":
        F = 0
    elif what == "Fin=0":
        Fin = 0
    elif what == "ldg<Fin":
        ld = 5
    elif what == "res=3":
        res = 3
    else:
        rp, res = None, (P.RES_MEAN if what.endswith("MEAN") else P.RES_PROJ)
    errs = _refused(entry, "gat_unfold_grads", INVALID, {"g_fc_w": g_fc, "g_res_fc_w": g_res}, gW.ptr(), a.ptr(),
                    H, F, Fin, ld, res, g_fc.ptr(), rp, stream_ptr())
    assert not errs, errs


# ====================================================================== 4. mvml_gat_attn_grad
def _attn_grad_run(c, inp):
    L = lib()
    Y = Placed((1, c.N, c.HF), c.HF + c.pad_y, 0, 0, 1, inp["Y"])
    ge = Placed((1, c.N, 2 * c.H), 2 * c.H + c.pad_g, 0, 0, 1, inp["gelr"])
    gl, gr = Placed((1, 1, c.HF), c.HF), Placed((1, 1, c.HF), c.HF)
    wsz = L.mvml_gat_attn_grad_workspace_size(c.N, c.H, c.F)
    S = P.attn_grad_plan(c.N, c.HF)[0]
    assert wsz >= S * 2 * c.HF * 4 and wsz % 4 == 0, (wsz, S)
    ws = Placed((1, 1, wsz // 4), wsz // 4)      # exactly the advertised size, inside poison
    call("mvml_gat_attn_grad", c.N, c.H, c.F, Y.ptr(), Y.ld, ge.ptr(), ge.ld, gl.ptr(), gr.ptr(), ws.ptr(), wsz,
         stream_ptr())
    torch.cuda.synchronize()
    return gl, gr, ws


@pytest.mark.parametrize("kind", ["a", "b"])
def test_attn_grad(kind):
    fails = []
    for c in P.ATTN_GRAD_CASES:
        inp = P.attn_grad_inputs(c, kind)
        res, errs = _guard(lambda: _attn_grad_run(c, inp), c.name)
        if res is not None:
            gl, gr, ws = res
            for n, pl in (("g_attn_l", gl), ("g_attn_r", gr), ("workspace", ws)):
                _outside(n, pl, errs)
            got = torch.stack([gl.read()[0, 0], gr.read()[0, 0]])
            _finite("g_attn", got, errs)
            ref, den = P.attn_grad_reference(c, inp["Y"], inp["gelr"])
            if kind == "a":
                _exact("g_attn", got, ref, errs)
            else:
                _held("g_attn", c.name, "attn_grad", got, ref, den, c.depth * P.U, errs)
        fails += [f"{c.name}: {m}" for m in errs]
    _report(fails, len(P.ATTN_GRAD_CASES))


@pytest.mark.parametrize("what", ["ldy<HF", "ldgl<2H", "workspace short", "workspace NULL"])
def test_attn_grad_refusals(what):
    N, H, F = 5, 2, 4
    Y, ge = Placed((1, N, 8), 8, data=torch.ones(N, 8)), Placed((1, N, 4), 4, data=torch.ones(N, 4))
    gl, gr = Placed((1, 1, 8), 8), Placed((1, 1, 8), 8)
    wsz = lib().mvml_gat_attn_grad_workspace_size(N, H, F)
    ws = Placed((1, 1, wsz // 4), wsz // 4)
    ldy, ldgl, wp, wn, code = 8, 4, ws.ptr(), wsz, INVALID
    if what == "ldy<HF":
        ldy = 7
    elif what == "ldgl<2H":
        ldgl = 3
    elif what == "workspace short":
        wn, code = wsz - 1, WORKSPACE
    else:
        wp, code = None, WORKSPACE
    errs = _refused("mvml_gat_attn_grad", "gat_attn_grad", code, {"g_attn_l": gl, "g_attn_r": gr, "workspace": ws},
                    N, H, F, Y.ptr(), ldy, ge.ptr(), ldgl, gl.ptr(), gr.ptr(), wp, wn, stream_ptr())
    assert not errs, errs


# ====================================================================== 5. head mean
def _head_mean_run(c, inp):
    HF = c.H * c.F
    X = Placed((1, c.N, HF), HF + c.pad_x, 0, 0, 1, inp["X"])
    R = Placed((1, c.N, c.F), c.F + c.pad_r, 0, 0, 1)
    gR = Placed((1, c.N, c.F), c.F + c.pad_r, 0, 0, 1, inp["gR"])
    gX = Placed((1, c.N, HF), HF + c.pad_x, 0, 0, 1)
    call("mvml_head_mean_f32", c.N, c.H, c.F, X.ptr(), X.ld, R.ptr(), R.ld, stream_ptr())
    call("mvml_head_mean_bwd_f32", c.N, c.H, c.F, gR.ptr(), gR.ld, gX.ptr(), gX.ld, stream_ptr())
    torch.cuda.synchronize()
    return R, gX


@pytest.mark.parametrize("kind", ["a", "b"])
@pytest.mark.parametrize("H", [1, 2, 3, 4, 8])
def test_head_mean(H, kind):
    cases = [c for c in P.HEAD_MEAN_CASES if c.H == H]
    fails = []
    for c in cases:
        inp = P.head_mean_inputs(c, kind)
        res, errs = _guard(lambda: _head_mean_run(c, inp), c.name)
        if res is not None:
            R, gX = res
            _outside("R", R, errs)
            _outside("gX", gX, errs)
            r, gx = R.read()[0], gX.read()[0].reshape(c.N, c.H, c.F)
            _finite("R", r, errs)
            _finite("gX", gx, errs)
            ref, den = P.head_mean_reference(c, inp["X"])
            gref = (inp["gR"].double() / c.H)[:, None, :].expand(c.N, c.H, c.F)
            for h in range(1, c.H):
                _bitwise(f"gX head {h} vs head 0", gx[:, h], gx[:, 0], errs)
            if kind == "a":
                _exact("R", r, ref, errs)
                _exact("gX", gx, gref, errs)
            else:
                _held("R", c.name, "head_mean", r, ref, den, c.H * P.U, errs)
                if P.pow2(c.H):
                    _exact("gX", gx, gref, errs)          # an exact division: bitwise
                else:
                    _held("gX", c.name, "head_mean_bwd (H = 3)", gx, gref, gref.abs(), P.U, errs)
        fails += [f"{c.name}: {m}" for m in errs]
    _report(fails, len(cases))


@pytest.mark.parametrize("bwd", [0, 1])
@pytest.mark.parametrize("what", ["F%4", "wide stride%4", "narrow stride%4", "wide pointer", "narrow pointer",
                                  "wide stride<width", "narrow stride<width"])
def test_head_mean_refusals(bwd, what):
    N, H, F = 5, 2, 8
    off_w = 1 if what == "wide pointer" else 0      # 4 bytes off 16-B alignment, inside a valid buffer
    off_n = 1 if what == "narrow pointer" else 0
    wide = Placed((1, N, 16), 24, off_w, data=None if bwd else torch.ones(N, 16))
    narrow = Placed((1, N, 8), 16, off_n, data=torch.ones(N, 8) if bwd else None)
    ldw = {"wide stride%4": 18, "wide stride<width": 12}.get(what, 24)
    ldn = {"narrow stride%4": 10, "narrow stride<width": 4}.get(what, 16)
    if what == "F%4":
        F = 6
    if bwd:
        errs = _refused("mvml_head_mean_bwd_f32", "head_mean_bwd", INVALID, {"gX": wide}, N, H, F, narrow.ptr(), ldn,
                        wide.ptr(), ldw, stream_ptr())
    else:
        errs = _refused("mvml_head_mean_f32", "head_mean", INVALID, {"R": narrow}, N, H, F, wide.ptr(), ldw,
                        narrow.ptr(), ldn, stream_ptr())
    assert not errs, errs
