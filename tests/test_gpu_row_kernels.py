"""The small kernels every training step runs, at the ABI, against float64, element by element:
GraphNorm and the ReLU backward (csrc/norm.hip), LayerNorm rows, plain token attention and
BCE-with-logits (csrc/fusion_attn.hip), mvml_add_cols_f32 (csrc/gatv2_agg.hip) and the optimizer
pair (csrc/optim.hip).  _row_kernel_cases.py holds the tables, the references and the derivation
of every bar, test_row_kernel_cases_cpu.py the conditions that make them trustworthy, _placed.py the
poisoned buffers.

Every operand is a view into a larger device buffer of NaN poison.  After a call
 * every word outside the documented output region is bitwise the poison (pitch gaps, the other two
   views' rows of a 3 D pitch, tail rows, the workspace's tail, the pad floats between the
   optimizer's segments);
 * everything inside is finite (poison read as data would show as a NaN);
 * values are held element by element: bitwise (relu_bwd, add_cols, grad_gather, a skipped Adam
   parameter, every repeat run), GraphNorm to its fp64 bar, the fp32 kernels to max(4 e32, 8 u) den;
 * e, the bar and e / bar of every case go to parity_margins/row_kernels.json (MVML_MARGINS_DIR).
Every documented refusal (the table that passed on the CPU first) returns its code, names its entry
and leaves a poisoned pool untouched.  Several hundred small launches; seconds on an MI355X.
"""
import ctypes
import json
import os
import time

import pytest
import torch

import _row_kernel_cases as R
from _gemm_cases import POISON_BITS, first_diff
from _placed import DEV, MARGIN, Placed
from mvml_gat._lib import MvmlError, call, lib, stream_ptr

pytestmark = pytest.mark.gpu
MARGINS = {}
F32, F64 = torch.float32, torch.float64


def _p(t):
    return None if t is None else t.ptr()


def _where(count, idx):
    return f"{count} elements, first at {idx}"


def _bits(t):
    return t.contiguous().view(torch.int32)


def _untouched(name, pl, errs):
    n = int((pl.buf.view(torch.int32) != POISON_BITS).sum())
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


def _bitwise(name, got, want, errs):
    cnt, idx = first_diff(_bits(got), _bits(want))
    if cnt:
        errs.append(f"{name}: not bitwise equal: {_where(cnt, idx)}")


def _record(case, name, kernel, rec, ok, errs):
    MARGINS[f"{case}:{name}"] = dict(rec, kernel=kernel)
    if not ok:
        errs.append(f"{name}: outside its bar: {rec}")


def _held32(case, name, kernel, got, ref, den, r32, errs):
    rec, ok = R.fp32_check(got, ref, den, r32)
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
    """A dense [n] operand in poison."""
    n = data.numel() if data is not None else n
    return Placed((1, 1, n), n, data=data)


def _mat(rows, cols, ld, data=None):
    return Placed((1, rows, cols), ld, 0, 0, 1, data)


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
    with open(os.path.join(out, "row_kernels.json"), "w") as f:
        json.dump({"worst_e_over_bar": worst, "seconds": time.time() - t0, "cases": MARGINS}, f, indent=1)
    print("worst e / bar per kernel:", {k: round(v, 3) for k, v in sorted(worst.items())})
    print(f"test_gpu_row_kernels.py: {time.time() - t0:.1f} s")


# ====================================================================== GraphNorm
def _gn_fwd(c, inp, X, W, B, MS, off):
    N = inp["x"].shape[0]
    Y = _mat(N, c.D, c.D)
    call("mvml_graphnorm_fwd", c.G, c.D, ctypes.c_void_p(off.data_ptr()), X.ptr(), W.ptr(), B.ptr(), MS.ptr(),
         R.EPS32, Y.ptr(), stream_ptr())
    return Y


def _gn_bwd(c, inp, X, W, MS, GY, off, skip=None):
    N = inp["x"].shape[0]
    L = lib()
    wsz = L.mvml_graphnorm_bwd_workspace_size(c.G, c.D)
    assert wsz >= 3 * c.G * c.D * 8 and wsz % 4 == 0
    GX = _mat(N, c.D, c.D)
    outs = [None if skip == i else _vec(n=c.D) for i in range(3)]
    ws = _vec(n=wsz // 4)                                   # exactly the advertised size, poison after it
    call("mvml_graphnorm_bwd", c.G, c.D, ctypes.c_void_p(off.data_ptr()), X.ptr(), W.ptr(), MS.ptr(), R.EPS32,
         GY.ptr(), GX.ptr(), _p(outs[0]), _p(outs[1]), _p(outs[2]), ws.ptr(), wsz, stream_ptr())
    return GX, outs, ws


def _gn_case(c):
    inp = R.gn_inputs(c)
    N = inp["x"].shape[0]
    off = torch.tensor(inp["off"], dtype=torch.int64, device=DEV)
    X, GY = _mat(N, c.D, c.D, inp["x"]), _mat(N, c.D, c.D, inp["gy"])
    W, B, MS = _vec(inp["w"]), _vec(inp["b"]), _vec(inp["ms"])
    Y, Y2 = _gn_fwd(c, inp, X, W, B, MS, off), _gn_fwd(c, inp, X, W, B, MS, off)
    GX, outs, ws = _gn_bwd(c, inp, X, W, MS, GY, off)
    GX2, outs2, _ = _gn_bwd(c, inp, X, W, MS, GY, off)
    part = [_gn_bwd(c, inp, X, W, MS, GY, off, skip=i) for i in range(3)]
    torch.cuda.synchronize()
    errs = []
    pn = ("g_weight", "g_bias", "g_mean_scale")
    for n, pl in [("y", Y), ("g_x", GX), ("workspace", ws)] + list(zip(pn, outs)):
        _outside(n, pl, errs)
    _bitwise("y, second run", Y2.buf, Y.buf, errs)
    _bitwise("g_x, second run", GX2.buf, GX.buf, errs)
    for i in range(3):
        _bitwise(pn[i] + ", second run", outs2[i].buf, outs[i].buf, errs)
        gx_i, outs_i, ws_i = part[i]
        _outside(f"workspace without {pn[i]}", ws_i, errs)
        _bitwise(f"g_x without {pn[i]}", gx_i.buf, GX.buf, errs)
        for j in range(3):
            if j != i:
                _bitwise(f"{pn[j]} without {pn[i]}", outs_i[j].buf, outs[j].buf, errs)
    got = [Y.read()[0], GX.read()[0]] + [o.read()[0, 0] for o in outs]
    refs, dens = R.gn_eval(inp), R.gn_eval(inp, absolute=True)
    allowed = R.gn_bars(c, inp, refs, dens)
    for n, g, r, a in zip(("y", "g_x") + pn, got, refs, allowed):
        _finite(n, g, errs)
        rec, ok = R.allowed_check(g, r, a)
        _record(c.name, n, "graphnorm_fwd" if n == "y" else "graphnorm_bwd", rec, ok, errs)
    return errs


@pytest.mark.parametrize("pat", R.GN_PATTERNS, ids=lambda p: ".".join(p))
def test_graphnorm(pat):
    _run([c for c in R.GN_CASES if (c.xpat, c.mspat) == pat], _gn_case)


# ====================================================================== LayerNorm
def _ln_once(c, inp):
    X = _mat(c.rows, c.D, c.ld(0), inp["x"])
    GM, BT = _vec(inp["gamma"]), _vec(inp["beta"])
    Y, MEAN, RSTD = _mat(c.rows, c.D, c.ld(1)), _vec(n=c.rows), _vec(n=c.rows)
    call("mvml_layernorm_fwd", c.rows, c.D, X.ptr(), X.ld, GM.ptr(), BT.ptr(), R.EPS32, Y.ptr(), Y.ld, MEAN.ptr(),
         RSTD.ptr(), stream_ptr())
    MI, RI = _vec(inp["mean"]), _vec(inp["rstd"])
    GY = _mat(c.rows, c.D, c.ld(2), inp["gy"])
    GX, GYXH = _mat(c.rows, c.D, c.ld(3)), _mat(c.rows, c.D, c.D)
    call("mvml_layernorm_bwd", c.rows, c.D, X.ptr(), X.ld, GM.ptr(), MI.ptr(), RI.ptr(), GY.ptr(), GY.ld, GX.ptr(),
         GX.ld, GYXH.ptr(), stream_ptr())
    return {"y": Y, "mean": MEAN, "rstd": RSTD, "g_x": GX, "g_y_xhat": GYXH}


def _ln_case(c):
    inp = R.ln_inputs(c)
    out, out2 = _ln_once(c, inp), _ln_once(c, inp)
    torch.cuda.synchronize()
    errs = []
    fwd = dict(zip(("y", "mean", "rstd"), zip(R.ln_fwd(inp), R.ln_fwd(inp, absolute=True), R.ln_fwd(inp, F32))))
    bwd = dict(zip(("g_x", "g_y_xhat"), zip(R.ln_bwd(inp), R.ln_bwd(inp, absolute=True), R.ln_bwd(inp, F32))))
    for n, pl in out.items():
        _outside(n, pl, errs)
        _bitwise(n + ", second run", out2[n].buf, pl.buf, errs)
        got = pl.read()[0] if n in ("y", "g_x", "g_y_xhat") else pl.read()[0, 0]
        _finite(n, got, errs)
        ref, den, r32 = (fwd if n in fwd else bwd)[n]
        _held32(c.name, n, "layernorm_fwd" if n in fwd else "layernorm_bwd", got, ref, den, r32, errs)
    return errs


@pytest.mark.parametrize("pat", R.LN_PATTERNS)
def test_layernorm(pat):
    _run([c for c in R.LN_CASES if c.pat == pat], _ln_case)


# ====================================================================== plain token attention
def _at_once(c, inp):
    n_att, n_p = c.B * c.H * 3 * c.dk, c.B * c.H * 9
    QKV = _mat(3 * c.B, c.W, c.W + c.pad, inp["qkv"])
    ATT, P = _vec(n=n_att), _vec(n=n_p)
    call("mvml_token_attn_fwd", c.B, c.H, c.dk, QKV.ptr(), QKV.ld, inp["scale"], ATT.ptr(), P.ptr(), stream_ptr())
    PI, GA = _vec(inp["P32"].reshape(-1)), _vec(inp["g_att"].reshape(-1))
    G = _mat(3 * c.B, c.W, c.W + c.padg)
    call("mvml_token_attn_bwd", c.B, c.H, c.dk, QKV.ptr(), QKV.ld, inp["scale"], PI.ptr(), GA.ptr(), G.ptr(), G.ld,
         stream_ptr())
    return {"att": ATT, "P": P, "g_qkv": G}


def _at_case(c):
    inp = R.at_inputs(c)
    out, out2 = _at_once(c, inp), _at_once(c, inp)
    torch.cuda.synchronize()
    errs = []
    (att, P), (att_d, P_d), (att32, P32) = R.at_fwd(c, inp), R.at_fwd(c, inp, absolute=True), R.at_fwd(c, inp, F32)
    want = {"att": (att, att_d, att32), "P": (P, P_d, P32),
            "g_qkv": (R.at_bwd(c, inp), R.at_bwd(c, inp, absolute=True), R.at_bwd(c, inp, F32))}
    inst = "%s,%d" % R.by_width(c.dk)
    for n, pl in out.items():
        _outside(n, pl, errs)
        _bitwise(n + ", second run", out2[n].buf, pl.buf, errs)
        ref, den, r32 = want[n]
        got = pl.read()[0] if n == "g_qkv" else pl.read()[0, 0].reshape(ref.shape)
        _finite(n, got, errs)
        _held32(c.name, n, f"token_attn_{'bwd' if n == 'g_qkv' else 'fwd'}<{inst}>", got, ref, den, r32, errs)
    return errs


@pytest.mark.parametrize("pat", R.AT_PATTERNS)
def test_token_attn(pat):
    _run([c for c in R.AT_CASES if c.pat == pat], _at_case)


# ====================================================================== BCE with logits
def _bce_case(c):
    inp = R.bce_inputs(c)
    Z, Y = _vec(inp["z"]), _vec(inp["y"])
    outs = []
    for _ in range(2):
        LT, GZ = _vec(n=c.n), _vec(n=c.n)
        call("mvml_bce_logits", c.n, Z.ptr(), Y.ptr(), LT.ptr(), GZ.ptr(), stream_ptr())
        outs.append((LT, GZ))
    torch.cuda.synchronize()
    errs = []
    for i, n in enumerate(("loss_terms", "g_z")):
        pl = outs[0][i]
        _outside(n, pl, errs)
        _bitwise(n + ", second run", outs[1][i].buf, pl.buf, errs)
        got = pl.read()[0, 0]
        _finite(n, got, errs)
        _held32(c.name, n, "bce_logits", got, R.bce_eval(inp)[i], R.bce_eval(inp, absolute=True)[i],
                R.bce_eval(inp, F32)[i], errs)
    return errs


def test_bce_logits():
    _run(list(R.BCE_CASES), _bce_case)


# ====================================================================== relu_bwd, add_cols
def _relu_case(n):
    inp = R.relu_inputs(n)
    Y, GY = _vec(inp["y"]), _vec(inp["gy"])
    errs = []
    for s in R.RELU_SCALES:
        GX = _vec(n=n)
        call("mvml_relu_bwd", n, Y.ptr(), GY.ptr(), GX.ptr(), s, stream_ptr())
        torch.cuda.synchronize()
        _outside(f"g_x (scale {s})", GX, errs)
        _bitwise(f"g_x (scale {s})", GX.read()[0, 0], R.relu_expected(inp, s), errs)
    return errs


@pytest.mark.parametrize("n", R.RELU_N)
def test_relu_bwd(n):
    _run([n], lambda n_: _relu_case(n_))


def _add_cols_case(case):
    rows, cols, lds, ldd = case
    g = torch.Generator().manual_seed(rows * 1000 + cols + lds + ldd)
    src, dst = torch.randn(rows, cols, generator=g), torch.randn(rows, cols, generator=g)
    S, D = _mat(rows, cols, lds, src), _mat(rows, cols, ldd, dst)
    call("mvml_add_cols_f32", rows, cols, S.ptr(), lds, D.ptr(), ldd, stream_ptr())
    torch.cuda.synchronize()
    errs = []
    _outside("dst", D, errs)
    _bitwise("dst", D.read()[0], dst + src, errs)
    _bitwise("src", S.read()[0], src, errs)
    return errs


def test_add_cols():
    _run(list(R.ADD_COLS_CASES), _add_cols_case)


# ====================================================================== the optimizer pair
def _poison_host(n):
    return torch.full((n,), POISON_BITS, dtype=torch.int32)


class Flat:
    """A flat fp32 buffer [numel + extra] inside poison, with the host image of what it must hold."""

    def __init__(self, numel, extra=0):
        self.n = numel + extra
        self.image = _poison_host(MARGIN + self.n + MARGIN)

    def set(self, o, values):
        self.image[MARGIN + o:MARGIN + o + values.numel()] = values.contiguous().view(torch.int32)

    def upload(self):
        self.buf = self.image.to(DEV)
        return self

    def ptr(self, o=0):
        return ctypes.c_void_p(self.buf.data_ptr() + 4 * (MARGIN + o))

    def read(self):
        return self.buf.cpu()

    def seg(self, host_bits, o, n):
        return host_bits[MARGIN + o:MARGIN + o + n].view(torch.float32)


def _dev(vals, dtype):
    return torch.tensor(vals, dtype=dtype, device=DEV)


def _tables(c):
    cp, cb, ce, off, numel = R.opt_tables(c.sizes, c.chunk)
    assert R.tables_ok(c.sizes, cp, cb, ce, off, numel)
    return (_dev(cp, torch.int32), _dev(cb, torch.int64), _dev(ce, torch.int64), _dev(off, torch.int64)), off, numel


def _gather_case(c):
    """Sources in one poisoned buffer: every third NULL, every third 4 bytes off 16-B alignment."""
    (cp, cb, ce, po), off, numel = _tables(c)
    ps = R.opt_inputs(c)
    src_off, o = [], 0
    for i, q in enumerate(ps):
        o = (o + 3) // 4 * 4 + 4 + (1 if i % 3 == 2 else 0)
        src_off.append(o)
        o += q["g"].numel()
    SRC = Flat(o + 4)
    want = Flat(numel, c.P)
    for i, q in enumerate(ps):
        null = i % 3 == 1
        if not null:
            SRC.set(src_off[i], q["g"])
        want.set(off[i], torch.zeros_like(q["g"]) if null else q["g"])
        want.set(numel + i, torch.tensor([0.0 if null else 1.0]))
    SRC.upload()
    tab = _dev([0 if i % 3 == 1 else SRC.buf.data_ptr() + 4 * (MARGIN + src_off[i]) for i in range(c.P)], torch.int64)
    errs = []
    outs = []
    for _ in range(2):
        flat = Flat(numel, c.P).upload()
        call("mvml_grad_gather", len(cp), ctypes.c_void_p(cp.data_ptr()), ctypes.c_void_p(cb.data_ptr()),
             ctypes.c_void_p(ce.data_ptr()), ctypes.c_void_p(po.data_ptr()), ctypes.c_void_p(tab.data_ptr()), c.P,
             flat.ptr(), numel, stream_ptr())
        outs.append(flat)
    torch.cuda.synchronize()
    # the whole buffer: gradients, zeros for NULL sources, flags, and poison in every pad and margin
    _bitwise("flat | flags | pads", outs[0].read(), want.image, errs)
    _bitwise("second run", outs[1].read(), outs[0].read(), errs)
    _bitwise("sources", SRC.read(), SRC.image, errs)
    return errs


def test_grad_gather():
    seen, cases = set(), []
    for c in R.OPT_CASES:                                   # one per (layout, chunk length)
        if (c.layout, c.chunk) not in seen:
            seen.add((c.layout, c.chunk))
            cases.append(c)
    _run(cases, _gather_case)


def _adam_case(c):
    (cp, cb, ce, po), off, numel = _tables(c)
    ps = R.opt_inputs(c)
    bufs = {k: Flat(numel) for k in "pgmv"}
    for q, o in zip(ps, off):
        for k in "pgmv":
            bufs[k].set(o, q[k])
    flags = _vec(torch.tensor([q["flag"] for q in ps]))
    steps0 = [q["step"] for q in ps]
    runs = []
    for _ in range(2):
        b = {k: Flat(numel) for k in "pgmv"}
        for k in "pgmv":
            b[k].image = bufs[k].image.clone()
            b[k].upload()
        steps = _dev(steps0, torch.int32)
        call("mvml_adam_flat", len(cp), ctypes.c_void_p(cp.data_ptr()), ctypes.c_void_p(cb.data_ptr()),
             ctypes.c_void_p(ce.data_ptr()), flags.ptr(), ctypes.c_void_p(steps.data_ptr()), c.P, b["p"].ptr(),
             b["g"].ptr(), b["m"].ptr(), b["v"].ptr(), c.lr, c.betas[0], c.betas[1], c.eps, c.wd, c.gs, stream_ptr())
        runs.append((b, steps))
    torch.cuda.synchronize()
    errs = []
    b, steps = runs[0]
    got = {k: b[k].read() for k in "pgmv"}
    for k in "pmv":
        _bitwise(f"{k}, second run", runs[1][0][k].read(), got[k], errs)
    _bitwise("steps, second run", runs[1][1].cpu(), steps.cpu(), errs)
    _bitwise("grad (an input)", got["g"], bufs["g"].image, errs)
    _untouched_flags = []
    _outside("flags", flags, _untouched_flags)
    errs += _untouched_flags
    want_steps = [s + (1 if q["flag"] > 0 else 0) for s, q in zip(steps0, ps)]
    if steps.cpu().tolist() != want_steps:
        errs.append("step counters: not exactly one higher where the flag is > 0 and unchanged elsewhere")
    # outside the live segments (pads, margins, skipped parameters): bitwise what went in
    live = torch.zeros(bufs["p"].image.numel(), dtype=torch.bool)
    for q, o in zip(ps, off):
        if q["flag"] > 0:
            live[MARGIN + o:MARGIN + o + q["p"].numel()] = True
    for k in "pmv":
        cnt, idx = first_diff(got[k][~live], bufs[k].image[~live])
        if cnt:
            errs.append(f"{k}: {cnt} words changed outside the updated parameters (pads, margins, flag-0 parameters)")
    cat = {k: ([], [], [], []) for k in "pmv"}
    for q, o in zip(ps, off):
        if q["flag"] > 0 and q["p"].numel():
            ref, den, r32 = R.adam_eval(c, q), R.adam_eval(c, q, absolute=True), R.adam_eval(c, q, F32)
            for j, k in enumerate("pmv"):
                for lst, t in zip(cat[k], (b[k].seg(got[k], o, q["p"].numel()), ref[j], den[j], r32[j])):
                    lst.append(t)
    for k, name in zip("pmv", ("param", "exp_avg", "exp_avg_sq")):
        g_, ref, den, r32 = (torch.cat(t) for t in cat[k])
        _finite(name, g_, errs)
        _held32(c.name, name, "adam_flat", g_, ref, den, r32, errs)
    return errs


@pytest.mark.parametrize("layout", list(R.OPT_LAYOUTS))
def test_adam_flat(layout):
    _run([c for c in R.OPT_CASES if c.layout == layout], _adam_case)


def test_flat_adam_tables_satisfy_the_contract():
    """FlatAdam's own chunk table at parameters around the chunk length: exact tiling, no straddling,
    offsets % 4 == 0."""
    from mvml_gat.optim import FlatAdam
    sizes = (16383, 16384, 16385, 3)
    params = [torch.nn.Parameter(torch.zeros(n, device=DEV)) for n in sizes]
    opt = FlatAdam(params)
    cp, cb, ce, off = (t.cpu().tolist() for t in (opt.chunk_param, opt.chunk_beg, opt.chunk_end, opt.param_off))
    assert opt.nchunks == len(cp) == 5
    assert R.tables_ok(sizes, cp, cb, ce, off, opt.numel)
    assert all(o % 4 == 0 for o in off) and opt.numel % 4 == 0 and opt.gbuf.numel() == opt.numel + len(sizes)


# ====================================================================== the refusals
@pytest.fixture(scope="module")
def pool():
    return Placed((1, 1, 1 << 16), 1 << 16)                 # every pointer of a refused call; never followed


def test_refusals_leave_poison(pool):
    """The table test_row_kernel_cases_cpu.py passed without a GPU, with every pointer inside one
    poisoned buffer: the code, the entry's name, and not one word written."""
    base = pool.buf.data_ptr() + 4 * pool.start
    table = R.refusals(ctypes.c_void_p(base), ctypes.c_void_p(base + 4))
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
    _untouched("the pool", pool, fails)
    assert not fails, fails
