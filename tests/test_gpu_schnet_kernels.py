"""The SchNet kernels (csrc/schnet.hip) at the ABI, against float64, element by element: the fused
filter forward and backward, the W_1 gradient, the aggregation in both directions and the ssp pair.
_schnet_cases.py holds the tables, the references and the derivation of every bar,
test_schnet_cases_cpu.py the conditions that make them trustworthy, _placed.py the poisoned buffers.

Every operand, the weight image and the workspace are views into larger device buffers of NaN
poison.  After a call
 * every word outside the documented output region is bitwise the poison (pitch gaps, the row past
   E, the bytes past the image, the workspace's tail) and every input is bitwise what went in;
 * everything inside is finite; a second run is bitwise equal;
 * values are held element by element: by value where the inputs make the result exact, the fp32
   kernels to max(4 e32, 8 u) den, the split-fp16 products to their propagated allowance;
 * e, the bar and e / bar of every case go to parity_margins/schnet_kernels.json (MVML_MARGINS_DIR).
A tile-unaligned sub-range of the slots, or one atom's list, run alone gives the same bits.  Every
documented refusal (the table that passed on the CPU first) returns its code, names its entry and
leaves a poisoned pool untouched.  Several hundred small launches; seconds on an MI355X.
"""
import ctypes
import json
import os
import time

import pytest
import torch

import _schnet_cases as S
import _schnet_ref as SR
from _gemm_cases import POISON_BITS, first_diff
from _placed import DEV, Placed
from mvml_gat._lib import MvmlError, call, lib, stream_ptr

pytestmark = pytest.mark.gpu
MARGINS = {}
F32, F64 = torch.float32, torch.float64


def _where(count, idx):
    return f"{count} elements, first at {idx}"


def _bits(t):
    return t.contiguous().view(torch.int32)


def _outside(name, pl, errs):
    n, pos = pl.outside()
    if n:
        errs.append(f"{name}: written outside its region: {_where(n, pos)}")


def _finite(name, got, errs):
    nf = ~torch.isfinite(got)
    if bool(nf.any()):
        errs.append(f"{name}: non-finite: {_where(int(nf.sum()), tuple(nf.nonzero()[0].tolist()))}")


def _bitwise(name, got, want, errs):
    cnt, idx = first_diff(_bits(got), _bits(want))
    if cnt:
        errs.append(f"{name}: not bitwise equal: {_where(cnt, idx)}")


def _same_values(name, got, want, errs):
    cnt, idx = first_diff(got, want)
    if cnt:
        errs.append(f"{name}: not exactly the float64 result: {_where(cnt, idx)}")


def _unchanged(name, pl, before, errs):
    """An input: the whole buffer (operand, gaps, margins) is bitwise what it was."""
    _bitwise(name + " (an input)", pl.buf, before, errs)


def _record(case, name, kernel, rec, ok, errs):
    MARGINS[f"{case}:{name}"] = dict(rec, kernel=kernel)
    if not ok:
        errs.append(f"{name}: outside its bar: {rec}")


def _held32(case, name, kernel, got, ref, den, r32, errs):
    rec, ok = S.fp32_check(got, ref, den, r32)
    _record(case, name, kernel, rec, ok, errs)


def _allowed(case, name, kernel, got, ref, allowed, errs):
    rec, ok = S.allowed_check(got, ref, allowed)
    _record(case, name, kernel, rec, ok, errs)


def _guard(fn, name):
    """Run one case: a refused call or a failed check is a failure of the case, a device error ends
    the session (nothing more is launched on this GPU)."""
    try:
        return fn()
    except (MvmlError, AssertionError) as err:
        return [f"{type(err).__name__}: {err}"]
    except RuntimeError as err:
        pytest.exit(f"device error in {name}: {err}", returncode=3)


def _run(cases, fn):
    fails = []
    for c in cases:
        name = c if isinstance(c, str) else getattr(c, "name", str(c))
        fails += [f"{name}: {m}" for m in _guard(lambda: fn(c), name)]
    assert not fails, f"{len(fails)} failures in {len(cases)} cases:\n" + "\n".join(fails[:40])


def _vec(data=None, n=None):
    n = data.numel() if data is not None else n
    return Placed((1, 1, n), n, data=data)


def _ivec(data):
    """int32 values in poison."""
    pl = Placed((1, 1, data.numel()), data.numel())
    pl.buf.view(torch.int32)[pl.idx.reshape(-1).to(DEV)] = data.to(DEV, torch.int32)
    return pl


def _mat(rows, cols, ld, data=None):
    return Placed((1, rows, cols), ld, 0, 0, 1, data)       # one tail row: the row past the last is poison


def _col(data, ld):
    """d: one float per slot at a stride of ld floats."""
    return Placed((1, data.numel(), 1), ld, data=data)


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
        r = max(rec["ratio"], rec.get("ratio_floor", 0.0))
        worst[rec["kernel"]] = max(worst.get(rec["kernel"], 0.0), r)
    with open(os.path.join(out, "schnet_kernels.json"), "w") as f:
        json.dump({"worst_e_over_bar": worst, "seconds": time.time() - t0, "cases": MARGINS}, f, indent=1)
    print("worst e / bar per kernel:", {k: round(v, 3) for k, v in sorted(worst.items())})
    print(f"test_gpu_schnet_kernels.py: {time.time() - t0:.1f} s")


# ====================================================================== the weight image
def _image(H, K, W1, W2):
    nb = lib().mvml_schnet_image_bytes(H, K)
    assert nb == S.image_bytes(H, K) and nb % 16 == 0
    IMG, PW1, PW2 = _vec(n=nb // 4), _vec(W1.reshape(-1)), _vec(W2.reshape(-1))
    call("mvml_schnet_split_w", H, K, PW1.ptr(), PW2.ptr(), IMG.ptr(), stream_ptr())
    return IMG, PW1, PW2


def _image_case(case):
    H, K, kind = case
    g = torch.Generator().manual_seed(H * 1000 + K)
    W1, W2 = torch.randn((H, K), generator=g) * 3.0, torch.randn((H, H), generator=g) / 7.0
    if kind == "zero":
        W1 = torch.zeros(H, K)
    IMG, PW1, PW2 = _image(H, K, W1, W2)
    w1b, w2b = PW1.buf.clone(), PW2.buf.clone()
    IMG2, _, _ = _image(H, K, W1, W2)
    torch.cuda.synchronize()
    errs = []
    _outside("image", IMG, errs)                            # the bytes past mvml_schnet_image_bytes
    _unchanged("W1", PW1, w1b, errs)
    _unchanged("W2", PW2, w2b, errs)
    words = IMG.read(torch.int32)[0, 0]
    _bitwise("amax words", words[:2], torch.stack([W1.abs().max(), W2.abs().max()]), errs)
    # (the header's other words are not documented either way: not held)
    body, body2 = words[64:], IMG2.read(torch.int32)[0, 0][64:]
    if bool((body == POISON_BITS).any()):
        errs.append("image: words inside it left unwritten")
    if bool((body2 != body).any()):
        errs.append("image: second run differs")
    halves = body.view(torch.float16)
    _finite("image", halves.float(), errs)
    if kind == "zero" and bool(halves[:S.sn_ks(K) * (H // 16) * 128 * 8].any()):
        errs.append("image: W_1 = 0 gives a non-zero W_1 image")
    return errs


def test_split_image():
    _run([(16, 1, "rand"), (32, 33, "rand"), (64, 300, "zero"), (80, 31, "rand"), (112, 512, "rand"), (128, 64, "zero")],
         _image_case)


# ====================================================================== the filter, forward
def _fwd_once(c, inp, IMG, d=None):
    d = inp["d"] if d is None else d
    E = d.numel()
    ops = {"d": _col(d, c.ldd), "centers": _vec(inp["centers"]), "b1": _vec(inp["b1"]), "b2": _vec(inp["b2"])}
    before = {k: v.buf.clone() for k, v in ops.items()}
    out = {"s1": _mat(E, c.H, c.ld(0)), "he": _mat(E, c.H, c.ld(1))}
    call("mvml_schnet_filter_fwd", E, ops["d"].ptr(), c.ldd, ops["centers"].ptr(), c.K, inp["gamma"], c.H, IMG.ptr(),
         ops["b1"].ptr(), ops["b2"].ptr(), out["s1"].ptr(), out["s1"].ld, out["he"].ptr(), out["he"].ld, stream_ptr())
    return out, ops, before


def _fwd_case(c, regime):
    inp = S.filter_inputs(c, regime)
    IMG, _, _ = _image(c.H, c.K, inp["W1"], inp["W2"])
    img0 = IMG.buf.clone()
    out, ops, before = _fwd_once(c, inp, IMG)
    out2, _, _ = _fwd_once(c, inp, IMG)
    torch.cuda.synchronize()
    errs = []
    _unchanged("image", IMG, img0, errs)
    for k, pl in ops.items():
        _unchanged(k, pl, before[k], errs)
    ref, _, allowed, _ = S.fwd_bars(inp)
    inst = f"filter_fwd<{c.ntb}>"
    got = {}
    for k, pl in out.items():
        _outside(k, pl, errs)
        _bitwise(k + ", second run", out2[k].buf, pl.buf, errs)
        got[k] = pl.read()[0]
        _finite(k, got[k], errs)
        _allowed(c.name + "/" + regime, k, f"{inst}:{k}", got[k], ref[k], allowed[k], errs)
    if regime in ("zero_w1", "zero_w2"):                    # row-independent: every row is row 0, bit for bit
        k = "s1" if regime == "zero_w1" else "he"
        _bitwise(f"{k} rows under a zero weight", got[k], got[k][:1].expand(c.E, c.H), errs)
    if regime == "onehot":                                  # pre1 is exact: s1 at the fp32 ssp bar of that value
        pre1 = ref["pre1"]
        _held32(c.name + "/onehot", "s1 (exact pre1)", f"{inst}:s1 onehot", got["s1"], SR.ssp(pre1), S._sp(pre1.abs()),
                SR.ssp(pre1.float()), errs)
    return errs


@pytest.mark.parametrize("regime", S.REGIMES)
def test_filter_fwd(regime):
    _run(list(S.regime_cases(regime)), lambda c: _fwd_case(c, regime))


# ====================================================================== the filter, backward
def _bwd_once(c, inp, IMG, s1, he, sl=slice(None)):
    E = s1[sl].shape[0]
    ops = {"src": _ivec(inp["src"][sl]), "dst": _ivec(inp["dst"][sl]), "dA": _mat(S.NODES, c.H, c.ld(2), inp["dA"]),
           "hv": _mat(S.NODES, c.H, c.ld(3), inp["hv"]), "s1": _mat(E, c.H, c.ld(0), s1[sl]), "he": _mat(E, c.H, c.ld(1), he[sl])}
    before = {k: v.buf.clone() for k, v in ops.items()}
    out = {"dpre2": _mat(E, c.H, c.ld(4)), "dpre1": _mat(E, c.H, c.ld(5))}
    call("mvml_schnet_filter_bwd", E, ops["src"].ptr(), ops["dst"].ptr(), ops["dA"].ptr(), ops["dA"].ld, ops["hv"].ptr(),
         ops["hv"].ld, ops["s1"].ptr(), ops["s1"].ld, ops["he"].ptr(), ops["he"].ld, c.H, c.K, IMG.ptr(), out["dpre2"].ptr(),
         out["dpre2"].ld, out["dpre1"].ptr(), out["dpre1"].ld, stream_ptr())
    return out, ops, before


def _bwd_case(c, regime):
    if regime == "exact2":
        inp, s1, he = S.exact2_inputs(c)
    else:
        inp = S.filter_inputs(c, regime)
        s1, he = S.bwd_given(inp)
    IMG, _, _ = _image(c.H, c.K, inp["W1"], inp["W2"])
    img0 = IMG.buf.clone()
    out, ops, before = _bwd_once(c, inp, IMG, s1, he)
    out2, _, _ = _bwd_once(c, inp, IMG, s1, he)
    torch.cuda.synchronize()
    errs = []
    _unchanged("image", IMG, img0, errs)
    for k, pl in ops.items():
        _unchanged(k, pl, before[k], errs)
    got = {}
    for k, pl in out.items():
        _outside(k, pl, errs)
        _bitwise(k + ", second run", out2[k].buf, pl.buf, errs)
        got[k] = pl.read()[0]
        _finite(k, got[k], errs)
    inst = f"filter_bwd<{c.ntb}>"
    if regime == "exact2":
        for k, want in zip(("dpre2", "dpre1"), S.exact2_expected(inp)):
            _same_values(k, got[k], want, errs)
    else:
        ref, den, r32_2, allowed, _ = S.bwd_bars(inp, s1, he)
        _held32(c.name + "/" + regime, "dpre2", inst + ":dpre2", got["dpre2"], ref[0], den[0], r32_2, errs)
        _allowed(c.name + "/" + regime, "dpre1", inst + ":dpre1", got["dpre1"], ref[1], allowed, errs)
    if regime in ("rows", "exact2"):                        # a zero dA row: exactly 0
        z = inp["dst"] == S.ZERO_ROW
        for k in got:
            if bool((got[k][z] != 0).any()):
                errs.append(f"{k}: not exactly 0 under an all-zero dA row")
    return errs


@pytest.mark.parametrize("regime", S.REGIMES + ("exact2",))
def test_filter_bwd(regime):
    cases = S.regime_cases("rows" if regime == "exact2" else regime)
    if regime == "exact2":                                  # every width once more: W_2^T's image at each H
        cases = cases + tuple(c for c in S.F_CASES if c.H not in {x.H for x in cases})
    _run(list(cases), lambda c: _bwd_case(c, regime))


# ====================================================================== dW_1
def _dw1_once(c, inp):
    L = lib()
    wsz = L.mvml_schnet_dw1_workspace_size(c.E, c.H, c.K)
    assert wsz == S.dw1_workspace(c.E, c.H, c.K) and wsz % 4 == 0
    ops = {"d": _col(inp["d"], c.ldd), "centers": _vec(inp["centers"]), "dpre1": _mat(c.E, c.H, c.H + c.pad, inp["dpre1"])}
    before = {k: v.buf.clone() for k, v in ops.items()}
    DW = _mat(c.H, c.K, c.K, inp["base"] if c.accumulate else None)   # (not accumulating: onto poison)
    ws = _vec(n=wsz // 4)                                    # exactly the advertised size, poison after it
    call("mvml_schnet_dw1", c.E, ops["d"].ptr(), c.ldd, ops["centers"].ptr(), c.K, inp["gamma"], ops["dpre1"].ptr(),
         ops["dpre1"].ld, c.H, c.accumulate, DW.ptr(), ws.ptr(), wsz, stream_ptr())
    return DW, ws, ops, before


def _dw1_case(c):
    inp = S.dw1_inputs(c)
    DW, ws, ops, before = _dw1_once(c, inp)
    DW2, _, _, _ = _dw1_once(c, inp)
    torch.cuda.synchronize()
    errs = []
    for k, pl in ops.items():
        _unchanged(k, pl, before[k], errs)
    _outside("dW1", DW, errs)
    _outside("workspace", ws, errs)
    _bitwise("dW1, second run", DW2.buf, DW.buf, errs)
    got = DW.read()[0]
    _finite("dW1", got, errs)
    _held32(c.name, "dW1", "dw1", got, S.dw1_eval(c, inp), S.dw1_eval(c, inp, absolute=True), S.dw1_eval(c, inp, F32), errs)
    return errs


def test_dw1():
    _run(list(S.D_CASES), _dw1_case)


# ====================================================================== the aggregation
def _agg_once(c, inp, N=None, rowptr=None, widx=None):
    N = c.N if N is None else N
    rowptr = inp["rowptr"] if rowptr is None else rowptr
    widx = inp["widx"] if widx is None else widx
    ops = {"rowptr": _ivec(rowptr), "xidx": _ivec(inp["xidx"]), "X": _mat(c.N + 2, c.H, c.H + c.pads[0], inp["X"]),
           "Wt": _mat(inp["E"], c.H, c.H + c.pads[1], inp["Wt"])}
    if widx is not None:
        ops["widx"] = _ivec(widx)
    before = {k: v.buf.clone() for k, v in ops.items()}
    OUT = _mat(N, c.H, c.H + c.pads[2])
    call("mvml_cfconv_agg", N, inp["E"], ops["rowptr"].ptr(), ops["widx"].ptr() if widx is not None else None,
         ops["xidx"].ptr(), ops["X"].ptr(), ops["X"].ld, ops["Wt"].ptr(), ops["Wt"].ld, c.H, OUT.ptr(), OUT.ld, stream_ptr())
    return OUT, ops, before


def _agg_case(c):
    errs = []
    for exact in (False, True):
        tag = "exact" if exact else "real"
        inp = S.agg_inputs(c, exact)
        OUT, ops, before = _agg_once(c, inp)
        OUT2, _, _ = _agg_once(c, inp)
        # one atom's list alone: the longest, as a one-row CSR over the same arrays
        v = max(range(c.N), key=lambda i: (c.degrees[i], i))
        b, e = int(inp["rowptr"][v]), int(inp["rowptr"][v + 1])
        w = torch.arange(b, e, dtype=torch.int32) if inp["widx"] is None else inp["widx"][b:e]
        ONE, _, _ = _agg_once(c, inp, 1, torch.tensor([0, e - b], dtype=torch.int32), w)
        torch.cuda.synchronize()
        for k, pl in ops.items():
            _unchanged(f"{tag} {k}", pl, before[k], errs)
        _outside(tag + " out", OUT, errs)
        _outside(tag + " out of one list", ONE, errs)
        _bitwise(tag + " out, second run", OUT2.buf, OUT.buf, errs)
        got = OUT.read()[0]
        _finite(tag + " out", got, errs)
        _bitwise(f"{tag} atom {v} alone", ONE.read()[0, 0], got[v], errs)
        empty = [i for i, n in enumerate(c.degrees) if n == 0]
        _bitwise(tag + " empty lists (+0)", got[empty], torch.zeros(len(empty), c.H), errs)
        ref = S.agg_eval(c, inp)
        if exact:
            _same_values("exact out", got, ref.float(), errs)
        else:
            _held32(c.name, "out", f"cfconv_agg<{S.agg_instance(c.H)}>", got, ref, S.agg_eval(c, inp, absolute=True),
                    S.agg_eval(c, inp, F32), errs)
    return errs


@pytest.mark.parametrize("direction", S.A_DIRS)
def test_cfconv_agg(direction):
    _run([c for c in S.A_CASES if c.direction == direction], _agg_case)


# ====================================================================== ssp
def _ssp_case(c):
    inp = S.ssp_inputs(c)
    runs = []
    for _ in range(2):
        X, Yin, GY = _vec(inp["x"]), _vec(inp["y"]), _vec(inp["gy"])
        Y = X if c.inplace else _vec(n=c.n)
        GX = GY if c.inplace else _vec(n=c.n)
        call("mvml_ssp_fwd", c.n, X.ptr(), Y.ptr(), stream_ptr())
        call("mvml_ssp_bwd", c.n, Yin.ptr(), GY.ptr(), GX.ptr(), stream_ptr())
        runs.append((X, Yin, GY, Y, GX))
    torch.cuda.synchronize()
    errs = []
    X, Yin, GY, Y, GX = runs[0]
    _bitwise("y (ssp_bwd's input)", Yin.read()[0, 0], inp["y"], errs)
    if not c.inplace:
        _bitwise("x (an input)", X.read()[0, 0], inp["x"], errs)
        _bitwise("g_y (an input)", GY.read()[0, 0], inp["gy"], errs)
    for n, pl, other in (("x", X, runs[1][0]), ("y in", Yin, runs[1][1]), ("g_y", GY, runs[1][2]), ("y", Y, runs[1][3]),
                         ("g_x", GX, runs[1][4])):
        _outside(n, pl, errs)
        _bitwise(n + ", second run", other.buf, pl.buf, errs)
    y, gx = Y.read()[0, 0], GX.read()[0, 0]
    _finite("y", y, errs)
    _finite("g_x", gx, errs)
    _held32(c.name, "y", "ssp_fwd", y, S.ssp_fwd(inp), S.ssp_fwd(inp, absolute=True), S.ssp_fwd(inp, F32), errs)
    _held32(c.name, "g_x", "ssp_bwd", gx, S.ssp_bwd(inp), S.ssp_bwd(inp, absolute=True), S.ssp_bwd(inp, F32), errs)
    return errs


def test_ssp():
    _run(list(S.S_CASES), _ssp_case)


# ====================================================================== batch independence at the ABI
def _independence_case(c):
    """The slots [e0, e1), neither a tile boundary, run alone: the same s1 / he / dpre2 / dpre1 bits."""
    inp = S.filter_inputs(c, "rows")
    e0, e1 = (37, c.E - 5) if c.E > 50 else (1, c.E - 2)
    assert 0 < e0 < e1 < c.E and e0 % 16 and e1 % 16
    sl = slice(e0, e1)
    IMG, _, _ = _image(c.H, c.K, inp["W1"], inp["W2"])
    full, _, _ = _fwd_once(c, inp, IMG)
    part, _, _ = _fwd_once(c, inp, IMG, inp["d"][sl])
    s1, he = S.bwd_given(inp)
    bfull, _, _ = _bwd_once(c, inp, IMG, s1, he)
    bpart, _, _ = _bwd_once(c, inp, IMG, s1, he, sl)
    torch.cuda.synchronize()
    errs = []
    for k in ("s1", "he"):
        _outside(k + " of the sub-range", part[k], errs)
        _bitwise(f"{k} of slots [{e0}, {e1}) alone", part[k].read()[0], full[k].read()[0][sl], errs)
    for k in ("dpre2", "dpre1"):
        _outside(k + " of the sub-range", bpart[k], errs)
        _bitwise(f"{k} of slots [{e0}, {e1}) alone", bpart[k].read()[0], bfull[k].read()[0][sl], errs)
    return errs


def test_a_sub_range_alone_gives_the_same_bits():
    _run([c for c in S.regime_cases("rows") if c.E >= 15], _independence_case)


# ====================================================================== the refusals
@pytest.fixture(scope="module")
def pool():
    return Placed((1, 1, 1 << 16), 1 << 16)                 # every pointer of a refused call; never followed


def test_refusals_leave_poison(pool):
    """The table test_schnet_cases_cpu.py passed without a GPU, with every pointer inside one poisoned
    buffer: the code, the entry's name, and not one word written."""
    base = pool.buf.data_ptr() + 4 * pool.start
    table = S.refusals(ctypes.c_void_p(base), ctypes.c_void_p(base + 4))
    L = lib()
    fails = []
    for what, (entry, who, code, args) in table.items():
        args = list(args[:-1]) + [stream_ptr()]
        rc = getattr(L, entry)(*args)
        msg = L.mvml_last_error().decode(errors="replace")
        if rc != code or who not in msg:
            fails.append(f"{what}: returned {rc} ({msg!r}), expected {code} naming {who}")
            break                                          # nothing more is sent after a call that was not refused
    try:
        torch.cuda.synchronize()
    except RuntimeError as err:
        pytest.exit(f"device error after a refusal: {err}", returncode=3)
    n = int((pool.buf.view(torch.int32) != POISON_BITS).sum())
    if n:
        fails.append(f"the pool: {n} words written where nothing may be")
    assert not fails, fails
