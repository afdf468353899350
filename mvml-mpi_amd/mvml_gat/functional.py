"""torch.autograd.Functions over the HIP kernels of libmvml_gat.so.

Each Function owns one stage of GNNModule (model.py:89-95) and calls only the C ABI; there is
no PyTorch math on the hot path besides allocation (and nn.Dropout, which the reference
applies with torch's own RNG, model.py:87).
"""
import collections
import contextlib
import ctypes
import os

import numpy as np
import torch

from . import _lib
from ._lib import call, ptr

MODE_FLATTEN_ELU, MODE_MEAN, MODE_FLATTEN = 0, 1, 2
# residual kinds of a GAT layer (dgl 0.9.1 GATConv.__init__): res_fc a bias-free Linear, the
# identity (in_feats == H * F), or absent (residual=False); include/mvml_gat.h MVML_RES_*
RES_PROJ, RES_IDENTITY, RES_NONE = "proj", "identity", "none"
_MVML_RES_NONE = 2


def _check_cuda_f32(t, name):
    if not t.is_cuda:
        raise RuntimeError(f"{name} must be a CUDA (HIP) tensor: the mvml_gat path has no CPU fallback")
    if t.dtype != torch.float32:
        raise TypeError(f"{name} must be float32, got {t.dtype}")


def _c(t):
    return t if t.is_contiguous() else t.contiguous()


def _stream(dev):
    return _lib.stream_ptr(dev)


_UNIT_SEGMENT = {}


def _unit_segment(dev):
    """int64 [0, 1] on `dev` (made once): the offsets of one one-element segment."""
    t = _UNIT_SEGMENT.get(str(dev))
    if t is None:
        t = _UNIT_SEGMENT[str(dev)] = torch.tensor([0, 1], dtype=torch.int64, device=dev)
    return t


def zeros(shape, dtype=torch.float32, device=None):
    """torch.zeros through mvml_fill_zero (hipMemsetAsync): no framework fill kernel in the step."""
    t = torch.empty(shape, dtype=dtype, device=device)
    zero_(t)
    return t


def zero_(t):
    """Zero a contiguous tensor, or a 2-D row-pitched one (unit column stride), in place."""
    es = t.element_size()
    if t.is_contiguous():
        n = t.numel() * es
        call("mvml_fill_zero", ptr(t), 1, n, n, _stream(t.device))
    else:
        if t.dim() != 2 or t.stride(1) != 1:
            raise ValueError("zero_: contiguous or 2-D row-pitched tensors only")
        call("mvml_fill_zero", ptr(t), t.shape[0], t.shape[1] * es, t.stride(0) * es, _stream(t.device))
    return t


def copy2d(dst, src):
    """dst[:] = src for float32 2-D views with unit column stride (1-D: one row); a src row
    stride of 0 (an expanded row) replicates it (mvml_copy_cols)."""
    d2 = dst.view(1, -1) if dst.dim() == 1 else dst
    s2 = src.reshape(1, -1) if src.dim() == 1 else src
    if d2.shape != s2.shape or d2.stride(1) != 1 or (s2.shape[1] > 1 and s2.stride(1) != 1):
        raise ValueError("copy2d: matching 2-D views with unit column stride")
    call("mvml_copy_cols", d2.shape[0], d2.shape[1], ptr(s2), s2.stride(0) if s2.shape[0] > 1 else s2.shape[1],
         ptr(d2), d2.stride(0) if d2.shape[0] > 1 else d2.shape[1], _stream(dst.device))
    return dst


# Diagnostics hook (tools/diag_golden.py, the parity tests' kink-branch capture): when a dict,
# GATLayerFunction.forward appends each layer's el/er to DEBUG_CAPTURE["elr_fwd"] and the
# backward stores its saved el/er, attention and el/er gradients; LinearReLUFunction appends its
# post-ReLU output to ["relu_out"], the fusion its Conv2d+ReLU output to ["conv_out"] and
# WeightedSumAndMaxFunction its forward's argmax to ["readout_argmax"]; SAGEConvFunction appends its
# post-ReLU output to ["sage_out"], fc_pool's to ["sage_pool"] and the neighbour maximum's owner
# slots to ["sage_arg"]; GINLayerFunction appends its MLP's post-ReLU hidden rows to ["gin_hidden"]
# and a ReLU layer's output (before its Dropout) to ["gin_out"], SegmentPoolFunction the max
# readout's argmax to ["pool_argmax"].  None in normal use.
DEBUG_CAPTURE = None


def _round4(x):
    return (x + 3) // 4 * 4


# Row pitch of the N-row projection / gradient matrices: a multiple of 64 floats, so every row
# starts on a 256-B boundary and the aggregation kernels' 64-column chunks (256-B row segments)
# never straddle an extra cache line
def _row_pitch(cols):
    return (cols + 63) // 64 * 64


def agg_fwd_bytes(N, E, H, F, out_cols, res_cols):
    """Algorithmic HBM bytes of one mvml_gat_agg_fwd: read Z and R once,
    rowptr, src ids, el/er; write the layer output and the saved attention.  R is the
    head-mean residual (F columns) in mean mode."""
    return 4 * (N * H * F + N * res_cols + 2 * N * H + (N + 1) + E + N * out_cols + E * H)


def agg_bwd_bytes(N, E, H, F, gout_cols, mode):
    """Algorithmic bytes of mvml_gat_agg_bwd: read Z, el/er, g_out (+ out for ELU'), the saved
    attention, both CSRs; write gY = [dZ_agg | dR | d el | d er]."""
    rw = F if mode == MODE_MEAN else H * F
    reads = N * H * F + 2 * N * H + N * gout_cols + (N * H * F if mode == 0 else 0) + E * H
    idx = 2 * (N + 1) + 3 * E
    writes = N * (H * F + rw + 2 * H)
    return 4 * (reads + idx + writes)


# GEMM algorithm for every dense product of the view: "f16x2" = scaled split-fp16 MFMA at fp32
# accuracy (mvml_gemm_f16x2, the default; 3 fp16 MFMAs per product), "x3" = split-bf16
# (mvml_gemm_f32x3, 6 bf16 MFMAs), "f32" = f32-input MFMA (mvml_gemm_f32).  All are parity-
# tested against fp64 at the fp32 bar; override with MVML_GEMM_ALGO=x3 / f32.
GEMM_ALGO = os.environ.get("MVML_GEMM_ALGO", "f16x2")
_GEMM_ENTRY = {"f32": ("mvml_gemm_f32", 0), "x3": ("mvml_gemm_f32x3", 1),
               "bf16": ("mvml_gemm_bf16", 2),  # bf16: the projection option of config 4
               "f16x2": ("mvml_gemm_f16x2", 3)}


# A record (_mvml_amax, _mvml_rows, _mvml_padded, _mvml_elu) is set by the producer on the exact
# tensor it wrote and trusted only while that tensor is unmodified by torch (same _version) and
# still is the storage the producer wrote (same data pointer, shape and strides) — a view, a copy
# or an in-place update through autograd-visible ops gets a fresh pass instead.
def _stamp(t):
    return t._version, t.data_ptr(), tuple(t.shape), t.stride()


def _remember(t, attr, *what):
    setattr(t, attr, (*what, _stamp(t)))


def _recall(t, attr):
    """What _remember put on t under attr (the stamp last), or None if nothing or t changed."""
    rec = getattr(t, attr, None)
    return rec if rec is not None and rec[-1] == _stamp(t) else None


def known_amax(X):
    """(int32 tensor, slot) holding max |X| bits if the kernel that produced X folded it into
    its stores (fold_amax) and X is unchanged since, else None."""
    rec = _recall(X, "_mvml_amax")
    return None if rec is None else rec[:2]


# Per-row A maxima (mvml_gemm_f16x2_rows): the split-fp16 products whose A rows are atoms or
# molecules split every row with its own scale — per-row fp32 accuracy, and a row's result
# independent of the batch it is computed in (a shard gives bitwise its slice of the whole
# batch).  MVML_ROW_SCALES=0: one scale per operand (the round-3 path).
ROW_SCALES = os.environ.get("MVML_ROW_SCALES", "1") != "0"


def known_rows(X):
    """Per-row |max| bits of X (int32 [rows]) if its producer recorded them (same rule as
    known_amax), else None."""
    rec = _recall(X, "_mvml_rows")
    return None if rec is None else rec[0]


def zero_padded(X, Fp):
    """The zero-padded [N, Fp] buffer X is the [:, :F] view of (batching.pad_columns: the
    batch's resident atom features), if unchanged since recorded, else None."""
    rec = _recall(X, "_mvml_padded")
    return rec[0] if rec is not None and rec[0].shape[1] == Fp else None


def fold_padded(out, buf):
    """Record that out is the [:, :F] view of the zero-padded buffer buf."""
    _remember(out, "_mvml_padded", buf)


def fold_rows(out, rows):
    """Record that rows[r] holds max |out[r, :]| bits (written with out by its producer)."""
    _remember(out, "_mvml_rows", rows)


def absmax_rows(P, rows, cols, ld, out=None, offset=0, accumulate=False):
    """out[r] (int32 [rows]) = bits of max_c |P[r, offset + c]| (mvml_absmax_rows_f32)."""
    if out is None:
        out = torch.empty(max(rows, 1), dtype=torch.int32, device=P.device)
    pp = ctypes.c_void_p(ptr(P).value + 4 * offset)
    call("mvml_absmax_rows_f32", rows, cols, pp, ld, ptr(out), int(accumulate), _stream(P.device))
    return out


def row_maxima(X, rows, cols, ld):
    """Per-row |max| bits of a K-contiguous operand: its producer's record, else one pass."""
    r = known_rows(X)
    return r if r is not None else absmax_rows(X, rows, cols, ld)


def _row_scales(X, A, N, K, amx, slot_idx=0):
    """Per-row |max| bits (int32 [N]) of the split-fp16 operand A [N, K]: the record X's producer
    left (A is X, or X with zero pad columns: the same row maxima), else one pass over A; their
    max, max |A|, goes to amx[slot_idx] (N floats read, not N x K)."""
    xr = known_rows(X)
    if xr is None:
        xr = absmax_rows(A, N, K, K)
    absmax(xr, N, 1, 1, amx, slot_idx)
    return xr


def fold_amax(out, amx, slot_idx):
    """Record that out's |max| bits are in amx[slot_idx] (folded by the kernel that wrote out)."""
    _remember(out, "_mvml_amax", amx, slot_idx)


def absmax(P, rows, cols, ld, out, slot=0, offset=0, accumulate=False):
    """out[slot] (int32 tensor) = bits of max |P[r, offset + c]| (mvml_absmax_f32)."""
    pp = ctypes.c_void_p(ptr(P).value + 4 * offset)
    op = ctypes.c_void_p(ptr(out).value + 4 * slot)
    call("mvml_absmax_f32", rows, cols, pp, ld, op, int(accumulate), _stream(out.device))


def slot(t, i):
    """Device pointer to element i of an int32 maxima tensor (None passes through)."""
    return None if t is None else ctypes.c_void_p(t.data_ptr() + 4 * i)


# Weights split ONCE per step into the interleaved-by-4 fp16 image (mvml_split_f16x2_il4) that
# the 256x256 split-fp16 tiles load in place of fp32 B: one 16-B load per piece as before and no
# split VALU for B (bitwise the in-kernel split).  MVML_BSPLIT_IL=0: every tile splits B itself.
BSPLIT_IL = os.environ.get("MVML_BSPLIT_IL", "1") != "0"


def split_il4(W, rows, cols, ld, amax_ptr):
    """W (fp32 [rows][ld]) as its interleaved split-fp16 image (same shape), or None when off,
    not the f16x2 algorithm, or not 16-B shaped."""
    if not BSPLIT_IL or GEMM_ALGO != "f16x2" or cols % 4 or ld % 4 or W.data_ptr() % 16:
        return None
    img = torch.empty((rows, ld), dtype=torch.float32, device=W.device)
    call("mvml_split_f16x2_il4", rows, cols, ptr(W), ld, amax_ptr, ptr(img), _stream(W.device))
    return img


def _split_weight(W, amx):
    """max |W| of the dense weight W into amx[1], and W's interleaved image made with it
    (split_il4; None where that does not apply)."""
    rows, cols = W.shape
    absmax(W, rows, cols, cols, amx, 1)
    return split_il4(W, rows, cols, cols, slot(amx, 1))


def split_il8(P, rows, K, ld, kmajor=0, amax_ptr=None, rows_max=None, out=None):
    """P's il8 split-fp16 image (mvml_split_f16x2_il8) for mvml_gemm_f16x2_planes: fp32
    [rows][K rounded up to 32]; x[r][k] = P[r, k] (kmajor 0) or P[k, r] (kmajor 1: the image of
    P^T); scale from amax_ptr (operand-wide) or rows_max (per row, int32 [rows])."""
    kp = (K + 31) // 32 * 32
    if out is None:
        out = torch.empty((max(rows, 1), kp), dtype=torch.float32, device=P.device)
    call("mvml_split_f16x2_il8", rows, K, ptr(P), ld, int(kmajor), amax_ptr, ptr(rows_max), ptr(out), kp,
         _stream(P.device))
    return out


def gemm_planes(A, M, N, K, lda, bimg, ldb, C, ldc, amax_b, amax_a=None, arows=None, a_image=False,
                bias=None, beta=0.0, act=0, role=None):
    """C[M,N] = act(A B^T + bias + beta C) with B given as its il8 image (split_il8, made with
    amax_b) and A fp32 (or, a_image, its il8 image made with the same maxima): the LDS-DMA
    split-fp16 tile (mvml_gemm_f16x2_planes).  amax_a: pointer to max |A| bits, or arows: per-row
    |A| max bits (int32 [M])."""
    _lib.call_tag[0] = {"flops": 2 * M * N * K, "shape": (M, N, K, 0, 0),
                        "bytes": 4 * (M * N + M * K + N * K), "role": role}
    call("mvml_gemm_f16x2_planes", M, N, K, ptr(A), lda, int(a_image), amax_a, ptr(arows), ptr(bimg), ldb,
         amax_b, ptr(bias), float(beta), int(act), ptr(C), ldc, _stream(C.device))


def gemm(A, B, M, N, K, a_kmajor, b_kmajor, lda, ldb, C, ldc, bias=None, beta=0.0, act=0, algo=None,
         amax=None, arows=None, bil4=None, role=None):
    """C[M,N] = act(A*B + bias + beta*C) on MFMA (see mvml_gemm_f32 / mvml_gemm_f32x3 /
    mvml_gemm_f16x2).  amax = (pointer to |A| max bits, pointer to |B| max bits) from absmax()
    lets split-fp16 products that share an operand share its max pass.  arows (split-fp16,
    K-contiguous A): per-row |A| max bits (int32 [M]) — every A row gets its own scale
    (mvml_gemm_f16x2_rows); amax then only needs B's pointer.  bil4: B's interleaved split
    image (split_il4, made with amax[1])."""
    # bytes: what the product must move at least (A, B and C once) — the small-K products
    # (layer 1's projection) are reported against HBM with it (bench.py roofline_proj_l1)
    _lib.call_tag[0] = {"flops": 2 * M * N * K, "shape": (M, N, K, int(a_kmajor), int(b_kmajor)),
                        "bytes": 4 * (M * N + M * K + N * K), "role": role}
    L = _lib.lib()
    dev = C.device
    wsz = L.mvml_gemm_workspace_size(M, N, K)
    wp, wn = _lib.ws_ptr_size(wsz, dev)
    algo = algo or GEMM_ALGO
    if algo == "f16x2" and arows is not None:
        if a_kmajor or amax is None or amax[1] is None:
            raise ValueError("gemm: per-row A maxima need a K-contiguous A and max |B|")
        # which kernel runs (the small-K memory kernel or the tile): bench.py files the timing
        # under the matching roofline
        fn = getattr(L, "mvml_gemm_rows_smallk", None)  # (absent from older libraries of A/B runs)
        sk = fn(int(b_kmajor), M, N, K, ptr(A), lda, ptr(bil4 if bil4 is not None else B), ldb, float(beta),
                int(act), ptr(C), ldc) if fn is not None else 0
        _lib.call_tag[0]["path"] = "smallk" if sk else "tile"
        call("mvml_gemm_f16x2_rows", M, N, K, ptr(A), lda, ptr(B), ldb, int(b_kmajor), ptr(bil4),
             ptr(arows), amax[1], ptr(bias), float(beta), int(act), ptr(C), ldc, wp, wn, _stream(dev))
        return
    if algo == "f16x2" and amax is not None and bil4 is not None:
        call("mvml_gemm_f16x2_bsplit", int(a_kmajor), int(b_kmajor), M, N, K, ptr(A), lda, ptr(B), ldb,
             ptr(bil4), 0, amax[0], amax[1], ptr(bias), float(beta), int(act), ptr(C), ldc, wp, wn,
             _stream(dev))
        return
    if algo == "f16x2" and amax is not None:
        call("mvml_gemm_f16x2_amax", int(a_kmajor), int(b_kmajor), M, N, K, ptr(A), lda, ptr(B), ldb,
             amax[0], amax[1], ptr(bias), float(beta), int(act), ptr(C), ldc, wp, wn, _stream(dev))
        return
    call(_GEMM_ENTRY[algo][0], int(a_kmajor), int(b_kmajor), M, N, K, ptr(A), lda,
         ptr(B), ldb, ptr(bias), float(beta), int(act), ptr(C), ldc, wp, wn, _stream(dev))


def gemm_batched(A, B, M, N, K, a_kmajor, b_kmajor, lda, ldb, C, ldc, batch, sa, sb, sc, beta=0.0):
    """C_z = A_z * B_z (+ beta C_z) for z < batch, operands at float strides sa / sb / sc
    (mvml_gemm_f32x3_batched: fp32-accurate split-bf16 MFMA, no split-K)."""
    _lib.call_tag[0] = {"flops": 2 * M * N * K * batch, "shape": (M, N, K, int(a_kmajor), int(b_kmajor), batch)}
    call("mvml_gemm_f32x3_batched", int(a_kmajor), int(b_kmajor), M, N, K, batch, ptr(A), lda, sa,
         ptr(B), ldb, sb, None, float(beta), 0, ptr(C), ldc, sc, _stream(C.device))


def colsum(X, M, N, ldx, out, beta=0.0, offset=0, alpha=1.0):
    """out = beta*out + alpha * column sums of X[:, offset:offset+N] (deterministic)."""
    L = _lib.lib()
    dev = out.device
    wp, wn = _lib.ws_ptr_size(L.mvml_colsum_workspace_size(M, N), dev)
    xp = ctypes.c_void_p(ptr(X).value + 4 * offset)
    call("mvml_colsum_f32", M, N, xp, ldx, float(alpha), float(beta), ptr(out), wp, wn, _stream(dev))


# Kernel paths picked per call from the batch's molecule sizes (host counts, no device work):
# "large" batches have half their atoms or more in molecules past the LDS molecule window
# (FLAT_SRC_MIN_ATOMS, gat_agg_common.h kWinL) — BASELINE config 5.
#  * Aggregation forward by destination wave (one wave per atom gathers whole projection rows
#    from L2; csrc/gat_agg_fwd.hip gat_agg_fwd_dst_kernel), every layer (MVML_DST_FWD_POLICY = all |
#    auto: the head-mean layer on large batches only | off): on small-molecule batches with the
#    edge softmax as its own launch first (dst_fwd = 2: 2.9 / 3.4 ms against the molecule
#    window's 3.5 / 3.7 at config 3), on large ones inside the wave (dst_fwd = 1: 4.5 / 6.2 ms
#    against 5.0 / 6.4 split, config 5) — MVML_DST_FWD_KIND forces one.
#  * Flatten layers' aggregation backward by source atom in one pass (option flat_src = 2,
#    gat_flat_bwd_src1_kernel) on large batches (MVML_FLAT_SRC_AUTO = 0 turns it off).
FLAT_SRC_AUTO = os.environ.get("MVML_FLAT_SRC_AUTO", "1") == "1"
FLAT_SRC_MIN_ATOMS = 128  # the LDS molecule window (gat_agg_common.h kWinL)
DST_FWD_POLICY = os.environ.get("MVML_DST_FWD_POLICY", "all")
DST_FWD_KIND = int(os.environ.get("MVML_DST_FWD_KIND", "0"))  # 0: by batch (see above)
#  * The ELU link (EluLink, below): the second layer's data-gradient GEMM applies ELU' in its
#    epilogue, so the first layer's backward gathers g_rst rows only (no `out` rows) — on large
#    batches, where that backward gathers rows per out-edge (flat_src); on small ones the
#    epilogue's extra read costs more than the molecule window saves (MVML_ELU_LINK = auto | on
#    | off).
ELU_LINK_POLICY = os.environ.get("MVML_ELU_LINK", "auto")


def _large_batch(g):
    return g.large_molecule_fraction(FLAT_SRC_MIN_ATOMS) >= 0.5


def _fwd_path(g, mode):
    """Context manager selecting the aggregation forward kernel path for this call."""
    dst = DST_FWD_POLICY == "all" or (DST_FWD_POLICY == "auto" and (mode != MODE_MEAN or _large_batch(g)))
    if not dst:
        return contextlib.nullcontext()
    return _lib.option("dst_fwd", DST_FWD_KIND or (1 if _large_batch(g) else 2))




class EluLink:
    """Fused ELU backward between two GAT layers of one GAT stack (mvml_gat.nn.GAT): the
    flatten + ELU layer's output records a link; the next layer's forward claims it, and its
    data-gradient GEMM then multiplies by ELU'(out) in its epilogue (act 3) and folds max |g|,
    so the first layer receives g_rst itself (no g_out * ELU' pass over N x H F).  The first
    layer's backward checks that the gradient it receives IS the one the claiming layer wrote."""

    __slots__ = ("claimed", "g_rst", "amax")

    def __init__(self, dev):
        self.claimed = False
        self.g_rst = None
        self.amax = zeros(1, dtype=torch.int32, device=dev)


# set by mvml_gat.nn.GAT.forward around its layer loop: links are made and claimed only there,
# where a flatten + ELU layer's output feeds exactly the next layer
ELU_LINK = [False]


def _elu_link_of(X):
    rec = _recall(X, "_mvml_elu")
    return None if rec is None else rec[0]


# ---- what GATLayerFunction and GATv2LayerFunction do alike ---------------------------------------
def _check_res_kind(who, res_kind, res_w):
    if res_kind not in (RES_PROJ, RES_IDENTITY, RES_NONE):
        raise ValueError(f"{who}: unknown residual kind {res_kind!r}")
    if (res_w is None) != (res_kind != RES_PROJ):
        raise ValueError(f"{who}: res_fc.weight goes with the projected residual only")


def _padded_input(X):
    """(X, Xp): X contiguous and Xp its GEMM operand, the feature dimension padded to a multiple
    of 4 (e.g. 74 atom features -> 76) so every operand row is 16-B aligned and the LDS-DMA path
    applies; pad columns are zero.  The batch's atom features may already sit in such a buffer
    (zero_padded): X then stays the view it is."""
    Xp = zero_padded(X, _round4(X.shape[1])) if X.dim() == 2 else None
    if Xp is None:
        X = _c(X)
        N, Fin = X.shape
        Xp = X if Fin % 4 == 0 else torch.nn.functional.pad(X, (0, _round4(Fin) - Fin))
    return X, Xp


def _identity_residual(Xp, H, F, mean, st):
    """(R, ldr) of an identity residual: the input itself, or its head mean in a head-mean layer."""
    N, Fp = Xp.shape
    if not mean:
        return Xp, Fp
    R = torch.empty((N, F), dtype=torch.float32, device=Xp.device)
    call("mvml_head_mean_f32", N, H, F, ptr(Xp), Fp, ptr(R), F, st)
    return R, F


def _head_mean_bias_grad(g_bias, N, H, F, G=None, ldg=0, offset=0):
    """Every head's bias of a head-mean layer sees g_out / H: one column sum (G's F columns at
    `offset`; G None: g_bias[:F] holds it already), replicated over the heads."""
    if G is not None:
        colsum(G, N, F, ldg, g_bias, offset=offset, alpha=1.0 / H)
    if H > 1:
        copy2d(g_bias.view(H, F)[1:], g_bias[:F].view(1, F).expand(H - 1, F))


def _new_gx(g_out, N, Fin, H, F, identity, st):
    """[N, Fin] for the data-gradient product; a head-mean layer's identity residual puts its
    share there first (g_out / H spread over the heads) and the product accumulates onto it."""
    gX = torch.empty((N, Fin), dtype=torch.float32, device=g_out.device)
    if identity:
        call("mvml_head_mean_bwd_f32", N, H, F, ptr(g_out), F, ptr(gX), Fin, st)
    return gX


class GATLayerFunction(torch.autograd.Function):
    """dgllife GATLayer(GATConv) forward/backward (model.py:79-81): projection GEMM (fc and
    res_fc as one MFMA GEMM) + fused el/er, edge-softmax, aggregation, residual, bias and
    flatten/ELU or head-mean kernel.

    res_kind: RES_PROJ (res_w = res_fc.weight: its rows ride in the projection GEMM),
    RES_IDENTITY (in_feats == H F: the input itself, or its head mean in a head-mean layer, is
    the residual; res_w None) or RES_NONE (res_w None).  bias may be None.  The identity / absent
    kinds build the narrower Wcat = [fc ; A_l ; A_r], Y = [Z | el | er] and gY = [dZ | d el | d er]
    and pass the residual to the aggregation as an input of its own (mvml_gat_agg_fwd_res /
    mvml_gat_agg_bwd_res); their parameters that do not exist get None gradients."""

    @staticmethod
    def forward(ctx, X, fc_w, res_w, attn_l, attn_r, bias, g, H, F, slope, mode, algo=None,
                res_kind=RES_PROJ):
        _check_res_kind("GATLayerFunction", res_kind, res_w)
        sep = res_kind != RES_PROJ  # no residual rows in Wcat / Y / gY
        if sep and (algo or GEMM_ALGO) == "bf16":
            raise NotImplementedError("GATLayerFunction: the bf16 projection needs a projected residual")
        for t, n in ((X, "feat"), (fc_w, "fc.weight"), (res_w, "res_fc.weight"), (bias, "bias")):
            if t is not None:
                _check_cuda_f32(t, n)
        # (A ones pad column that would make the dW GEMM emit the bias gradient as well was
        # measured 1.02e-5 from float64 on config 3 — the bias sums cancel and the split-fp16
        # representation error shows — so the bias keeps its exact fp32 column sum.)
        X, Xp = _padded_input(X)
        (N, Fin), Fp = X.shape, Xp.shape[1]
        dev = X.device
        HF = H * F
        if res_kind == RES_IDENTITY and Fin != HF:
            raise ValueError(f"GATLayerFunction: the identity residual needs in_feats == H F ({Fin} != {HF})")
        mean_res = int(mode == MODE_MEAN)
        C = HF if sep else _lib.lib().mvml_gat_proj_cols(H, F, mean_res)
        st = _stream(dev)
        attn_l, attn_r = _c(attn_l), _c(attn_r)
        HFa = attn_l.numel()
        attn_lr = torch.empty(2 * HFa, dtype=torch.float32, device=X.device)
        copy2d(attn_lr[:HFa], attn_l.reshape(-1))
        copy2d(attn_lr[HFa:], attn_r.reshape(-1))
        ctx.elu_claim = None
        link = _elu_link_of(X) if (ELU_LINK[0] and (algo or GEMM_ALGO) == "f16x2" and ROW_SCALES
                                   and X.requires_grad) else None
        # [fc.weight ; res_fc.weight (or its head mean) ; A_l ; A_r]: the projection GEMM uses
        # the first C rows, the backward all C + 2H (the el / er paths, see mvml_gat_agg_bwd)
        Wcat = torch.empty((C + 2 * H, Fp), dtype=torch.float32, device=dev)
        if sep:
            call("mvml_gat_fold_weights_res", ptr(_c(fc_w)), None, ptr(attn_lr), H, F, Fin, Fp,
                 _MVML_RES_NONE, ptr(Wcat), st)
        else:
            call("mvml_gat_fold_weights", ptr(_c(fc_w)), ptr(_c(res_w)), ptr(attn_lr), H, F, Fin, Fp,
                 mean_res, ptr(Wcat), st)
        L = _lib.lib()
        # split-fp16: |max| of X, Wcat (all C + 2H rows) and, in the backward, gY — each operand's
        # pass serves all of its products (projection, dL/dW, dL/dX)
        amx = None
        ax = None  # (tensor, slot) of max |X|
        xr = None  # per-row max |X| bits (ROW_SCALES)
        wil = None  # Wcat's interleaved split image (BSPLIT_IL)
        if (algo or GEMM_ALGO) == "f16x2":
            amx = zeros(4, dtype=torch.int32, device=dev)  # [X, Wcat, gY (bwd), out]
            if ROW_SCALES:
                # the projection splits every atom row with its own scale; max |X| (the weight
                # gradient's A-side scale) is the max of the row maxima (N floats, not N x Fp).
                # Layer 1's rows are those of the resident atom features (the pad columns are
                # zeros): computed once and recorded on the feature tensor itself.  (Xp's pad
                # columns are zeros: the whole padded row, float4 loads, has the same |max| as
                # its Fin features)
                xr = _row_scales(X, Xp, N, Fp, amx)
                if not X.requires_grad:
                    fold_rows(X, xr)
                ax = (amx, 0)
            else:
                ax = known_amax(Xp) if Xp is X else None  # layer 2: folded by layer 1's aggregation
            if ax is None:
                absmax(Xp, N, Fp, Fp, amx, 0)
                ax = (amx, 0)
            # Wcat split once: the projection's tiles and the backward's dL/dX read the image
            wil = _split_weight(Wcat, amx)
        # claim the previous layer's ELU link only where the fused data-gradient product will
        # run (per-row scales and the interleaved weight image: see backward).  An identity-
        # residual layer never claims: its residual's share of dL/dX is added to the product
        # (beta = 1), and the fused epilogue (mvml_gemm_f16x2_ex) has no accumulate, so ELU'
        # would not see the whole sum
        if (link is not None and not link.claimed and Fp == Fin and amx is not None
                and wil is not None and res_kind != RES_IDENTITY):
            link.claimed = True
            ctx.elu_claim = link
        if amx is not None or (algo or GEMM_ALGO) == "bf16":
            # el / er as 2H more GEMM columns: X [A_l ; A_r]^T with A_l[h] = sum_f attn_l[h, f]
            # fc.weight[h F + f] (Wcat's last 2H rows) — the same values re-associated, no
            # logit-partial epilogue and no finalize pass; then gathered into elr [N, 2H].  The
            # bf16 projection (config 4) takes the same path on the bf16-operand kernel: its C
            # tile leaves through the LDS epilogue instead of the logit-partial one's column
            # stores (9.5 -> ~5 ms per config-3 layer-2 launch)
            ldy = _row_pitch(C + 2 * H)
            Y = torch.empty((N, ldy), dtype=torch.float32, device=dev)
            if xr is not None:
                gemm(Xp, Wcat, N, C + 2 * H, Fp, 0, 0, Fp, Fp, Y, ldy, amax=(None, slot(amx, 1)),
                     arows=xr, bil4=wil, role="gat_proj")
            elif amx is not None:
                gemm(Xp, Wcat, N, C + 2 * H, Fp, 0, 0, Fp, Fp, Y, ldy, amax=(slot(*ax), slot(amx, 1)))
            else:
                gemm(Xp, Wcat, N, C + 2 * H, Fp, 0, 0, Fp, Fp, Y, ldy, algo="bf16")
            # (a native slice copy: torch's strided copy splits into 32-bit-indexable pieces,
            # 8 launches for a 1.75 M-atom batch)
            elr = torch.empty((N, 2 * H), dtype=torch.float32, device=dev)
            call("mvml_copy_cols", N, 2 * H, ptr(Y[:, C:]), ldy, ptr(elr), 2 * H, st)
        else:
            ldy = _row_pitch(C)
            Y = torch.empty((N, ldy), dtype=torch.float32, device=dev)
            elr = torch.empty((N, 2 * H), dtype=torch.float32, device=dev)
            wp, wn = _lib.ws_ptr_size(L.mvml_gat_proj_fwd_workspace_size(N, H, F), dev)
            _lib.call_tag[0] = {"flops": 2 * N * C * Fp}
            call("mvml_gat_proj_fwd", N, ptr(Xp), Fp, Fp, ptr(Wcat), Fp, ptr(attn_lr), H, F,
                 _MVML_RES_NONE if sep else mean_res,
                 _GEMM_ENTRY[algo or GEMM_ALGO][1], ptr(Y), ldy, ptr(elr), None, None, None, 0, wp, wn, st)
        out_cols = F if mode == MODE_MEAN else HF
        out = torch.empty((N, out_cols), dtype=torch.float32, device=dev)
        E = g.num_edges()
        attn = torch.empty((E, H), dtype=torch.float32, device=dev)
        # per-row max |out| for the consumer's per-row split-fp16 GEMMs (next layer, Set2Set)
        orows = torch.empty(max(N, 1), dtype=torch.int32, device=dev) if (amx is not None and ROW_SCALES) else None
        # the residual rows: Y's columns past H F (projected), the input itself or its head mean
        # (identity), or none
        rw = out_cols
        R, ldr = _identity_residual(Xp, H, F, mean_res, st) if res_kind == RES_IDENTITY else (None, 0)
        _lib.call_tag[0] = {"layer": f"H{H}xF{F}",
                            "bytes": agg_fwd_bytes(N, E, H, F, out_cols, 0 if res_kind == RES_NONE else rw)}
        with _fwd_path(g, mode):
            if not sep and bias is not None:
                call("mvml_gat_agg_fwd", N, ptr(g.node_groups), g.num_node_groups, ptr(g.in_rowptr),
                     ptr(g.in_src), ptr(Y), ldy, H, F, ptr(elr), ptr(_c(bias)), float(slope), int(mode),
                     ptr(out), ptr(attn), slot(amx, 3), ptr(orows), st)
            else:
                rp = ctypes.c_void_p(Y.data_ptr() + 4 * HF) if not sep else ptr(R)
                call("mvml_gat_agg_fwd_res", N, ptr(g.node_groups), g.num_node_groups, ptr(g.in_rowptr),
                     ptr(g.in_src), ptr(Y), ldy, H, F, ptr(elr), rp, ldr if sep else ldy,
                     ptr(_c(bias)) if bias is not None else None, float(slope), int(mode),
                     ptr(out), ptr(attn), slot(amx, 3), ptr(orows), st)
        if amx is not None:  # max |out| for the consumer's split-fp16 GEMMs (next layer, Set2Set)
            fold_amax(out, amx, 3)
        if orows is not None:
            fold_rows(out, orows)
        # flatten + ELU inside a GAT stack: the next layer's data-gradient GEMM may apply ELU'
        # in its epilogue (EluLink), so this layer's backward receives g_rst and reads no `out`
        ctx.link = None
        if (mode == MODE_FLATTEN_ELU and ELU_LINK[0] and amx is not None and ROW_SCALES
                and (ELU_LINK_POLICY == "on" or (ELU_LINK_POLICY == "auto" and _large_batch(g)))):
            ctx.link = EluLink(dev)
            _remember(out, "_mvml_elu", ctx.link)
        if DEBUG_CAPTURE is not None:
            DEBUG_CAPTURE.setdefault("elr_fwd", []).append(elr.detach().clone())
        ctx.save_for_backward(Xp, Wcat, Y, attn, elr, out, attn_l, attn_r, attn_lr)
        ctx.Fin = Fin
        ctx.g, ctx.H, ctx.F, ctx.slope, ctx.mode, ctx.ldy = g, H, F, slope, mode, ldy
        ctx.algo = algo
        ctx.res_kind, ctx.has_bias = res_kind, bias is not None
        ctx.amx = amx
        ctx.ax = ax
        ctx.wil = wil
        return out

    @staticmethod
    def backward(ctx, g_out):
        Xp, Wcat, Y, attn, elr, out, attn_l, attn_r, attn_lr = ctx.saved_tensors
        g, H, F, mode, ldy = ctx.g, ctx.H, ctx.F, ctx.mode, ctx.ldy
        link = ctx.link
        if link is not None and link.claimed:
            # the next layer's data-gradient GEMM applied ELU' already: g_out IS g_rst, and the
            # aggregation backward runs as plain flatten (mode 2: no ELU', no read of `out`)
            gr = link.g_rst
            if gr is None or g_out.data_ptr() != gr.data_ptr() or g_out.shape != gr.shape \
                    or g_out.stride() != gr.stride():
                raise RuntimeError("GAT ELU link: the gradient reaching the first layer is not the one "
                                   "the next layer's fused ELU backward wrote (was its output also "
                                   "consumed elsewhere?)")
            mode = MODE_FLATTEN
        g_out = _c(g_out)
        N, Fp = Xp.shape
        Fin = ctx.Fin
        dev = Xp.device
        HF = H * F
        mean_res = int(mode == MODE_MEAN)
        L = _lib.lib()
        res_kind, has_bias = ctx.res_kind, ctx.has_bias
        sep = res_kind != RES_PROJ
        C = HF if sep else L.mvml_gat_proj_cols(H, F, mean_res)
        CE = C + 2 * H  # + [d el | d er]
        ldg = _row_pitch(CE)
        st = _stream(dev)
        gY = torch.empty((N, ldg), dtype=torch.float32, device=dev)
        if ctx.amx is not None:
            zero_(ctx.amx[2:3])  # max |gY| of THIS backward (a second one, retain_graph, refolds it)
        wp, wn = _lib.ws_ptr_size(L.mvml_gat_agg_bwd_workspace_size(g.num_edges(), H), dev)
        # per-row max |gY| for the data-gradient product's per-row scales (not needed by layer 1,
        # whose input gradient is not formed)
        flat_src = FLAT_SRC_AUTO and mode != MODE_MEAN and _large_batch(g)
        gyr = None
        if ctx.amx is not None and ROW_SCALES and (ctx.needs_input_grad[0] or flat_src):
            # (the source-atom kernels then form max |gY| from the row maxima: no per-block atomics)
            gyr = torch.empty(max(N, 1), dtype=torch.int32, device=dev)
        _lib.call_tag[0] = {"layer": f"H{H}xF{F}",
                            "bytes": agg_bwd_bytes(N, g.num_edges(), H, F, g_out.shape[1], mode)}
        # Identity / absent residual: dR leaves through gR (mvml_gat_agg_bwd_res).  A flatten
        # layer's gR = g_rst is the identity residual's share of dL/dX — written straight into gX,
        # which the data-gradient product below then accumulates onto (beta = 1) — and its column
        # sums are the bias gradient (no residual but a bias: a scratch buffer; neither: not
        # formed).  A head-mean layer's dR is g_out itself, so nothing is formed there.
        gX = gR = None
        ldgr = 0
        if sep and mode != MODE_MEAN:
            if res_kind == RES_IDENTITY and ctx.needs_input_grad[0]:
                gX = torch.empty((N, Fin), dtype=torch.float32, device=dev)
                gR, ldgr = gX, Fin
            elif has_bias:
                gR, ldgr = torch.empty((N, HF), dtype=torch.float32, device=dev), HF
        with (_lib.option("flat_src", 2) if flat_src else contextlib.nullcontext()):
            if sep:
                call("mvml_gat_agg_bwd_res", N, ptr(g.node_groups), g.num_node_groups, ptr(g.in_rowptr),
                     ptr(g.in_src), ptr(g.out_rowptr), ptr(g.out_dst), ptr(g.out_inslot), ptr(Y), ldy,
                     ptr(elr), ptr(attn), ptr(out), ptr(g_out), H, F, float(ctx.slope), int(mode), ptr(gY),
                     ldg, C, ptr(gR), ldgr, slot(ctx.amx, 2), ptr(gyr), wp, wn, st)
            else:
                call("mvml_gat_agg_bwd", N, ptr(g.node_groups), g.num_node_groups, ptr(g.in_rowptr),
                     ptr(g.in_src), ptr(g.out_rowptr), ptr(g.out_dst), ptr(g.out_inslot), ptr(Y), ldy,
                     ptr(elr), ptr(attn), ptr(out), ptr(g_out), H, F, float(ctx.slope), int(mode), ptr(gY),
                     ldg, slot(ctx.amx, 2), ptr(gyr), wp, wn, st)
        amx = ctx.amx  # slot 2 = max |gY|, folded in by mvml_gat_agg_bwd's stores
        if DEBUG_CAPTURE is not None and amx is not None:
            DEBUG_CAPTURE.setdefault("gy_amax", []).append((gY[:, :CE].clone(), amx[2:3].clone()))
            if gyr is not None:
                DEBUG_CAPTURE.setdefault("gy_rows", []).append(gyr.clone())
        # dL/d[Wcat ; A_l ; A_r] = gY^T X  (split-K over atoms); the bias gradient is the column
        # sums of gY's residual columns (g_rst; mean: g_out / H for every head), formed with it
        # where the product's own reads can (mvml_gemm_f16x2_amax_colsum: layer 1)
        gW = torch.empty((CE, Fp), dtype=torch.float32, device=dev)
        g_bias = torch.empty((HF,), dtype=torch.float32, device=dev) if has_bias else None
        bias_done = False
        # (the fused column sums read gY's residual block: the projected layout with a bias only)
        if amx is not None and (ctx.algo or GEMM_ALGO) == "f16x2" and has_bias and \
                not sep and L.mvml_gemm_colsum_fused(CE, Fp, N):
            sum_n = F if mean_res else HF
            _lib.call_tag[0] = {"flops": 2 * CE * Fp * N, "shape": (CE, Fp, N, 1, 1),
                                "bytes": 4 * (CE * Fp + CE * N + Fp * N), "role": "gat_dw"}
            wp, wn = _lib.ws_ptr_size(L.mvml_gemm_colsum_workspace_size(CE, Fp, N, sum_n), dev)
            call("mvml_gemm_f16x2_amax_colsum", CE, Fp, N, ptr(gY), ldg, ptr(Xp), Fp, slot(amx, 2),
                 slot(*ctx.ax), ptr(gW), Fp, HF, sum_n, 1.0 / H if mean_res else 1.0, ptr(g_bias), wp, wn, st)
            bias_done = True
        else:
            gemm(gY, Xp, CE, Fp, N, 1, 1, ldg, Fp, gW, Fp, algo=ctx.algo,
                 amax=None if amx is None else (slot(amx, 2), slot(*ctx.ax)), role="gat_dw")
        g_fc = torch.empty((HF, Fin), dtype=torch.float32, device=dev)
        g_res = None
        if sep:
            call("mvml_gat_unfold_grads_res", ptr(gW), ptr(attn_lr), H, F, Fin, Fp, _MVML_RES_NONE,
                 ptr(g_fc), None, st)
        else:
            g_res = torch.empty((HF, Fin), dtype=torch.float32, device=dev)
            call("mvml_gat_unfold_grads", ptr(gW), ptr(attn_lr), H, F, Fin, Fp, mean_res, ptr(g_fc),
                 ptr(g_res), st)
        gelr = gY[:, C:CE]
        # dL/dattn_l[h, f] = sum_n d el[n, h] Z[n, h, f] = sum_k G_l[h, k] fc.weight[h F + f, k]
        # with G_l = [d el]^T X — rows C .. C+H of gW, already formed by the dW GEMM (and G_r
        # rows C+H ..): re-associated, a (2 x Fp) x (Fp x F) product per head instead of a pass
        # over the N x H F projection (mvml_gat_attn_grad, kept in the ABI)
        g_alr = torch.empty((2, HF), dtype=torch.float32, device=dev)
        gemm_batched(gW[C:], Wcat, 2, F, Fp, 0, 0, H * Fp, Fp, g_alr, HF, H, Fp, F * Fp, F)
        g_al = g_alr[0].view_as(attn_l)
        g_ar = g_alr[1].view_as(attn_r)
        if DEBUG_CAPTURE is not None:
            DEBUG_CAPTURE.update(elr=elr, gelr=gelr, attn=attn)
        if has_bias and mean_res:
            # (identity / absent residual: dR = g_out; the fused product has summed gY's already)
            _head_mean_bias_grad(g_bias, N, H, F, *((g_out, F) if sep else () if bias_done else (gY, ldg, HF)))
        elif has_bias and sep:  # (before the product below accumulates onto gR where it is gX)
            colsum(gR, N, HF, ldgr, g_bias)
        elif has_bias and not bias_done:
            colsum(gY, N, HF, ldg, g_bias, offset=HF)
        if ctx.needs_input_grad[0]:
            # the identity residual's share is in gX already (flatten: gR above; head mean:
            # g_out / H spread over the heads) and the product accumulates onto it
            beta = 1.0 if res_kind == RES_IDENTITY else 0.0
            if gX is None:
                gX = _new_gx(g_out, N, Fin, H, F, res_kind == RES_IDENTITY, st)
            link = ctx.elu_claim
            if link is not None and amx is not None and ROW_SCALES and ctx.wil is not None:
                # the previous layer's ELU backward in this product's epilogue: gX leaves as its
                # g_rst, with max |g_rst| folded for its GEMMs (EluLink)
                zero_(link.amax)
                _lib.call_tag[0] = {"flops": 2 * N * Fin * CE, "shape": (N, Fin, CE, 0, 1)}
                call("mvml_gemm_f16x2_ex", N, Fin, CE, 1, ptr(gY), ldg, 0, ptr(Wcat), Fp, 1, ptr(ctx.wil),
                     0, ptr(gyr if gyr is not None else absmax_rows(gY, N, CE, ldg)), 0, slot(amx, 1),
                     None, 0, 3, ptr(gX), Fin, 0, ptr(Xp), Fp, ptr(link.amax), None, 0, 0, 0, st)
                link.g_rst = gX
            elif amx is not None and ROW_SCALES:  # every atom's gradient row at its own scale
                gemm(gY, Wcat, N, Fin, CE, 0, 1, ldg, Fp, gX, Fin, amax=(None, slot(amx, 1)),
                     arows=gyr if gyr is not None else absmax_rows(gY, N, CE, ldg), bil4=ctx.wil, beta=beta)
            else:
                gemm(gY, Wcat, N, Fin, CE, 0, 1, ldg, Fp, gX, Fin, algo=ctx.algo,
                     amax=None if amx is None else (slot(amx, 2), slot(amx, 1)), beta=beta)
        else:
            gX = None
        return gX, g_fc, g_res, g_al, g_ar, g_bias, None, None, None, None, None, None, None


# Set2Set's gates GEMM + LSTM cell as one launch (mvml_lstm_gates_cell_fwd: the cell in the
# GEMM epilogue, interleaved weight rows) where the 256x256 plan applies; False: GEMM + cell
CELL_EPI = True


class Set2SetFunction(torch.autograd.Function):
    """dgl Set2Set.forward (model.py:92): n_iters x {n_layers LSTM cell steps, fused segment
    softmax readout}.  LSTM gates: one MFMA GEMM per cell over [x | h_prev] + pointwise kernel."""

    @staticmethod
    def forward(ctx, X, g, n_iters, n_layers, *lstm_params):
        _check_cuda_f32(X, "feat")
        X = _c(X)
        N, D = X.shape
        B = g.batch_size
        dev = X.device
        st = _stream(dev)
        T, Lr = n_iters, n_layers
        W = [tuple(_c(p) for p in lstm_params[4 * l:4 * l + 4]) for l in range(Lr)]  # w_ih, w_hh, b_ih, b_hh
        f32 = dict(dtype=torch.float32, device=dev)
        # Combined GEMM operands: XH[l][t] = [x_l(t) | h_l(t-1)] (kin_l + D columns) so each
        # cell's gates are ONE GEMM against [W_ih | W_hh]; layer 0's x is q*_{t-1}, so
        # XH[0][t+1][:, :2D] IS q*_t (the readout writes r_t there).  Each cell writes its h
        # twice: its own recurrence slot XH[l][t+1][:, kin:] and its consumer's input slot
        # (XH[l+1][t][:, :D], or q_t = XH[0][t+1][:, :D] for the top layer).
        kin = [2 * D] + [D] * (Lr - 1)
        XH = [torch.empty((T + 1, B, kin[l] + D), **f32) for l in range(Lr)]
        zero_(XH[0][0])
        for l in range(1, Lr):
            zero_(XH[l][0, :, D:])
        L = _lib.lib()
        # [W_ih | W_hh] and (cell epilogue) its interleaved rows: row 4 j + q = row q D + j (unit
        # j's i, f, g, o), both from one mvml_lstm_pack_weights launch per layer
        Wcat = [torch.empty((4 * D, kin[l] + D), **f32) for l in range(Lr)]
        Wperm = [torch.empty((4 * D, kin[l] + D), **f32) if CELL_EPI else None for l in range(Lr)]
        for l in range(Lr):
            call("mvml_lstm_pack_weights", D, kin[l], ptr(W[l][0]), ptr(W[l][1]), ptr(Wcat[l]), ptr(Wperm[l]), st)
        acts = torch.empty((T, Lr, B, 4 * D), **f32)
        cs = torch.empty((T, Lr, B, D), **f32)
        lse = torch.empty((T, B), **f32)
        gates = torch.empty((B, 4 * D), **f32)
        amax_x = amax_w = None
        mrows = None  # per-molecule bound of every cell's A row (ROW_SCALES)
        wsp = [(None, 0)] * Lr
        if GEMM_ALGO == "f16x2":
            # split-fp16 operand maxima of the cells' GEMMs: every A row [x | h_prev] holds
            # LSTM outputs h = o tanh(c) (|h| < 1) and, in layer 0, the readout r = sum_n a_n x_n
            # (a convex combination: |r| <= max |X|), so max(1, max |X|) bounds every cell's A
            # (an upper bound is all the scale needs) — one pass instead of one per cell
            kx = known_amax(X)  # folded by the last GAT layer's aggregation
            if kx is None:
                kx = (zeros(1, dtype=torch.int32, device=dev), 0)
                absmax(X, N, D, D, kx[0], 0, accumulate=True)
            # max(1, max |X|) on the float bits (non-negative: int order), one "segment" [0, 1)
            amax_x = torch.empty(1, dtype=torch.int32, device=dev)
            call("mvml_segment_max_bits", 1, ptr(_unit_segment(dev)), slot(*kx), 0x3F800000, ptr(amax_x), st)
            if ROW_SCALES:
                # per molecule: max(1, max |X| over its atoms) bounds every entry of its cell rows
                # [x | h] (h = o tanh c, the readout a convex combination of its own atoms' rows),
                # so a molecule's cells are split at a scale of its own
                xr = row_maxima(X, N, D, D)
                mrows = torch.empty(max(B, 1), dtype=torch.int32, device=dev)
                call("mvml_segment_max_bits", B, ptr(g.node_offsets), ptr(xr), 0x3F800000, ptr(mrows), st)
            amax_w = torch.empty(Lr, dtype=torch.int32, device=dev)
            for l in range(Lr):
                absmax(Wcat[l], 4 * D, kin[l] + D, kin[l] + D, amax_w, l)  # = Wperm's max
            # the gates' weights split once per forward into the interleaved image (the fused path
            # reads Wperm's, the unfused one Wcat's: the same values per element, so the same
            # products; w_plane = 0)
            wsp = [(split_il4(Wperm[l] if CELL_EPI else Wcat[l], 4 * D, kin[l] + D, kin[l] + D,
                              slot(amax_w, l)), 0) for l in range(Lr)]
        for t in range(T):
            for l in range(Lr):
                w_ih, w_hh, b_ih, b_hh = W[l]
                K = kin[l] + D if t > 0 else kin[l]  # h_l(-1) = 0: the recurrent half is skipped
                own = XH[l][t + 1][:, kin[l]:]
                nxt = XH[l + 1][t] if l < Lr - 1 else XH[0][t + 1]
                c_prev = cs[t - 1, l] if t > 0 else None
                ldn = kin[l + 1] + D if l < Lr - 1 else 3 * D
                if CELL_EPI and not (t == 0 and l == 0) and L.mvml_lstm_gates_cell_plan_ok(B, D, K):
                    pa = pw = None
                    if amax_x is not None:  # split-fp16: the operand maxima of this cell's GEMM
                        pa, pw = slot(amax_x, 0), slot(amax_w, l)
                    _lib.call_tag[0] = {"flops": 2 * B * 4 * D * K, "shape": (B, 4 * D, K, 0, 0, "cell")}
                    call("mvml_lstm_gates_cell_fwd", B, D, K, ptr(XH[l][t]), kin[l] + D, ptr(Wperm[l]),
                         kin[l] + D, ptr(b_ih), ptr(b_hh), ptr(c_prev), ptr(cs[t, l]), ptr(own),
                         kin[l] + D, ptr(acts[t, l]), ptr(nxt), ldn, pa, pw, ptr(mrows),
                         ptr(wsp[l][0]), wsp[l][1], st)
                    continue
                gp = gates
                if t == 0 and l == 0:
                    gp = None  # q*_{-1} = 0 and h_0(-1) = 0: zero pre-activations, the bias alone
                else:
                    gemm(XH[l][t], Wcat[l], B, 4 * D, K, 0, 0, kin[l] + D, kin[l] + D, gates, 4 * D,
                         amax=None if amax_x is None else (slot(amax_x, 0), slot(amax_w, l)),
                         arows=mrows,
                         bil4=wsp[l][0] if not CELL_EPI and wsp[l][1] == 0 else None)
                call("mvml_lstm_cell_fwd", B, D, ptr(gp), ptr(b_ih), ptr(b_hh), ptr(c_prev),
                     ptr(cs[t, l]), ptr(own), kin[l] + D, ptr(acts[t, l]), ptr(nxt), ldn, st)
            call("mvml_set2set_seg_fwd", B, D, ptr(g.node_offsets), ptr(X), ptr(XH[0][t + 1]), 3 * D,
                 ptr(lse[t]), st)
        ctx.save_for_backward(X, acts, cs, lse, *XH, *[p for w in W for p in w])
        ctx.g, ctx.T, ctx.Lr = g, T, Lr
        ctx.amax = (amax_x, amax_w)
        return copy2d(torch.empty((B, 2 * D), **f32), XH[0][T][:, :2 * D])

    @staticmethod
    def backward(ctx, g_out):
        X, acts, cs, lse, *rest = ctx.saved_tensors
        g, T, Lr = ctx.g, ctx.T, ctx.Lr
        XH, flat = rest[:Lr], rest[Lr:]
        W = [tuple(flat[4 * l:4 * l + 4]) for l in range(Lr)]
        qs = XH[0][1:]  # q*_t = XH[0][t+1][:, :2D], row stride 3D
        N, D = X.shape
        B = g.batch_size
        dev = X.device
        st = _stream(dev)
        f32 = dict(dtype=torch.float32, device=dev)
        # Recurrent data gradients as ONE GEMM per cell against [W_ih | W_hh] (4D x (kin+D)):
        # the outputs [dL/dx_l(t) | dL/dh_l(t-1)] land side by side — for layer 0 in the rows of
        # g_qs3[t-1] = [dL/dq*_{t-1} (2D) | dL/dh_0(t-1) (D)], for layers l > 0 in gxh[l] =
        # [dL/dh_{l-1}(t) | dL/dh_l(t-1)].  N = kin + D fills whole 256-column GEMM tiles
        # (768 / 1152) where two products of N = 384 would each waste a quarter of theirs.
        kins = [2 * D] + [D] * (Lr - 1)
        Wcat = [torch.empty((4 * D, kins[l] + D), **f32) for l in range(Lr)]
        for l in range(Lr):
            call("mvml_lstm_pack_weights", D, kins[l], ptr(W[l][0]), ptr(W[l][1]), ptr(Wcat[l]), None, st)
        g_qs3 = torch.empty((T, B, 3 * D), **f32)
        g_qstars = g_qs3[:, :, :2 * D]
        copy2d(g_qstars[T - 1], _c(g_out))
        alphas = torch.empty((T, N), **f32)
        g_es = torch.empty((T, N), **f32)
        gW_ih = [torch.empty_like(w[0]) for w in W]  # written below (one product per layer)
        gW_hh = [torch.empty_like(w[1]) for w in W]
        gb = [torch.empty_like(w[2]) for w in W]
        # every step's gate gradients are kept so that each weight gradient is ONE GEMM over
        # all T*B rows after the recurrence (K = 393k instead of 6 launches of 65k)
        g_gates_all = torch.empty((Lr, T, B, 4 * D), **f32)
        g_h = torch.empty((B, D), **f32)
        gxh = [None] + [torch.empty((B, 2 * D), **f32) for _ in range(1, Lr)]
        g_c = [torch.empty((B, D), **f32) for _ in range(Lr)]  # first read at t = T - 2 (None before)
        g_c_new = torch.empty((B, D), **f32)
        # LSTM bias gradients: every cell backward leaves [R, 4D] partial column sums of its
        # gate gradients (mvml_lstm_cell_bwd's gb_part); one column sum over the T R partial rows
        # per layer replaces a pass over all T B gate-gradient rows
        R = int(_lib.lib().mvml_lstm_cell_bwd_part_rows(B, D))
        gb_part = torch.empty((Lr, T, R, 4 * D), **f32)
        # split-fp16 maxima: the forward's bounds for XH (|x|, |h|) and [W_ih | W_hh], and a
        # running |max| of each layer's gate gradients, folded in by mvml_lstm_cell_bwd (the
        # running value bounds every cell seen so far, which is all a scale needs)
        amax_x, amax_w = ctx.amax
        amax_g = zeros(Lr, dtype=torch.int32, device=dev) if amax_x is not None else None
        wib = [None] * Lr  # [W_ih | W_hh] split once (interleaved image) for the per-cell data-gradient products
        if amax_g is not None:
            wib = [split_il4(Wcat[l], 4 * D, Wcat[l].shape[1], Wcat[l].shape[1], slot(amax_w, l))
                   for l in range(Lr)]
        for t in range(T - 1, -1, -1):
            # readout segment backward: dL/dq_t = g_qstar_t[:, :D] + segment term -> g_h
            call("mvml_set2set_seg_bwd", B, D, ptr(g.node_offsets), ptr(X), ptr(qs[t]), 3 * D,
                 ptr(lse[t]), ptr(g_qs3[t]), 3 * D, ptr(g_h), D, ptr(alphas[t]), ptr(g_es[t]), st)
            for l in range(Lr - 1, -1, -1):
                kin = 2 * D if l == 0 else D
                if l == Lr - 1:
                    gh, ldgh = g_h, D
                else:
                    gh, ldgh = gxh[l + 1][:, :D], 2 * D  # dL/dh_l(t) from layer l+1's input
                gh2, ldgh2 = None, 0
                if t < T - 1:  # + dL/dh_l(t) through the recurrence at step t+1 (summed in the kernel)
                    gh2, ldgh2 = (g_qs3[t][:, 2 * D:], 3 * D) if l == 0 else (gxh[l][:, D:], 2 * D)
                c_prev = cs[t - 1, l] if t > 0 else None
                g_gates = g_gates_all[l, t]
                call("mvml_lstm_cell_bwd", B, D, ptr(acts[t, l]), ptr(cs[t, l]), ptr(c_prev), ptr(gh), ldgh,
                     ptr(gh2), ldgh2,
                     ptr(g_c[l]) if t < T - 1 else None, ptr(g_gates), ptr(g_c_new), slot(amax_g, l),
                     ptr(gb_part[l, t]), st)
                g_c[l], g_c_new = g_c_new, g_c[l]
                # N = kin + D with the recurrent part (t > 0), kin alone at t = 0; layer 0 at
                # t = 0 has neither (its input q*_{-1} = 0 is a constant)
                ncols = kin + D if t > 0 else (kin if l > 0 else 0)
                if ncols:
                    out, ldo = (g_qs3[t - 1], 3 * D) if l == 0 else (gxh[l], 2 * D)
                    # (operand-wide scales here: GraphNorm's backward has already mixed each
                    # 64-molecule group's gradients, so the cells' rows span little)
                    gemm(g_gates, Wcat[l], B, ncols, 4 * D, 0, 1, 4 * D, kin + D, out, ldo,
                         amax=None if amax_g is None else (slot(amax_g, l), slot(amax_w, l)),
                         bil4=wib[l])
        # weight / bias gradients, one product per parameter over all steps:
        #   dW_ih[l] = sum_t g_gates[l,t]^T x_l(t),  dW_hh[l] = sum_{t>=1} g_gates[l,t]^T h_l(t-1)
        # (layer 0's input x_0(t) = q*_{t-1} is zero at t = 0; h_l(-1) = 0)
        # [dW_ih | dW_hh][l] = sum_t g_gates[l,t]^T XH[l][t] as ONE GEMM with N = kin + D: the
        # recurrent half of XH[l][0] is zero (h_l(-1) = 0) and for layer 0 the whole t = 0 block
        # is (q*_{-1} = 0), so it is skipped there.
        for l in range(Lr):
            G = g_gates_all[l]
            kin = 2 * D if l == 0 else D
            ldx = kin + D
            t0 = 1 if l == 0 else 0
            if T > t0:
                gWcat = torch.empty((4 * D, ldx), **f32)
                gemm(G[t0:], XH[l][t0:T], 4 * D, ldx, (T - t0) * B, 1, 1, 4 * D, ldx, gWcat, ldx,
                     amax=None if amax_g is None else (slot(amax_g, l), slot(amax_x, 0)))
                copy2d(gW_ih[l], gWcat[:, :kin])
                copy2d(gW_hh[l], gWcat[:, kin:])
            else:  # n_iters = 1: layer 0's only step reads q*_{-1} = 0 and h_0(-1) = 0
                zero_(gW_ih[l])
                zero_(gW_hh[l])
            colsum(gb_part[l], T * R, 4 * D, 4 * D, gb[l])
        gX = torch.empty((N, D), **f32)
        call("mvml_set2set_gx", N, D, T, ptr(g.node_graph), ptr(g.node_offsets), B, ptr(qs), 3 * D, B * 3 * D,
             ptr(g_qs3), 3 * D, B * 3 * D, ptr(alphas), ptr(g_es), ptr(gX), st)
        grads = []
        for l in range(Lr):
            grads += [gW_ih[l], gW_hh[l], gb[l], copy2d(torch.empty_like(gb[l]), gb[l])]
        return (gX, None, None, None, *grads)


def _rows_f32(t):
    """t as a float32 matrix the row-pitched kernels can read in place (unit column stride, a row
    stride and a base address that keep float4 accesses aligned), else a contiguous copy."""
    if t.dim() == 2 and t.stride(1) == 1 and t.stride(0) % 4 == 0 and t.stride(0) >= t.shape[1] \
            and t.data_ptr() % 16 == 0:
        return t
    return t.contiguous()


class WeightedSumAndMaxFunction(torch.autograd.Function):
    """dgllife WeightedSumAndMax.forward: [sum_nodes(sigmoid(Linear(x)) * x) | max_nodes(x)] in one
    pass over the atom rows (mvml_wsum_max_fwd), and its backward in one more (mvml_wsum_max_bwd
    plus the column sums of its partials for the gate's weight and bias).  weight [1, D], bias [1]
    (atom_weighting[0] of WeightAndSum); returns (B, 2 D)."""

    @staticmethod
    def forward(ctx, X, weight, bias, g):
        _check_cuda_f32(X, "feats")
        X = _rows_f32(X)
        N, D = X.shape
        B = g.batch_size
        dev = X.device
        weight, bias = _c(weight), _c(bias)
        out = torch.empty((B, 2 * D), dtype=torch.float32, device=dev)
        gate = torch.empty(N, dtype=torch.float32, device=dev)
        argmax = torch.empty((B, D), dtype=torch.int32, device=dev)
        if B == 0 or N == 0:  # no launch: every molecule is empty (sum 0, max 0, argmax -1)
            if B:
                zero_(out)
                argmax.fill_(-1)
        else:
            call("mvml_wsum_max_fwd", B, N, D, ptr(g.node_offsets), ptr(X), X.stride(0), ptr(weight),
                 ptr(bias), ptr(out), 2 * D, ptr(gate), ptr(argmax), D, _stream(dev))
        if DEBUG_CAPTURE is not None:  # the atoms the product took at the max's kinks (ties)
            DEBUG_CAPTURE.setdefault("readout_argmax", []).append(argmax.detach().clone())
        ctx.save_for_backward(X, weight, gate, argmax)
        ctx.g = g
        return out

    @staticmethod
    def backward(ctx, g_out):
        X, weight, gate, argmax = ctx.saved_tensors
        g = ctx.g
        N, D = X.shape
        B = g.batch_size
        dev = X.device
        g_out = _rows_f32(g_out)
        gX = torch.empty((N, D), dtype=torch.float32, device=dev)
        gW = torch.empty((1, D), dtype=torch.float32, device=dev)
        gb = torch.empty(1, dtype=torch.float32, device=dev)
        if B == 0 or N == 0:
            return gX, zero_(gW), zero_(gb), None
        R = _lib.lib().mvml_wsum_max_bwd_part_rows(B)
        ldp = D + 4
        part = torch.empty((R, ldp), dtype=torch.float32, device=dev)
        call("mvml_wsum_max_bwd", B, N, D, ptr(g.node_offsets), ptr(X), X.stride(0), ptr(weight),
             ptr(gate), ptr(argmax), D, ptr(g_out), g_out.stride(0), ptr(gX), D, ptr(part), ldp,
             _stream(dev))
        colsum(part, R, D, ldp, gW)
        colsum(part, R, 1, ldp, gb, offset=D)
        return gX, gW, gb, None


class GraphNormFunction(torch.autograd.Function):
    """torch_geometric GraphNorm.forward(x, batch=None) (model.py:93), per group."""

    @staticmethod
    def forward(ctx, x, weight, bias, mean_scale, group_offsets, eps):
        _check_cuda_f32(x, "x")
        x = _c(x)
        G = group_offsets.numel() - 1
        D = x.shape[1]
        y = torch.empty_like(x)
        call("mvml_graphnorm_fwd", G, D, ptr(group_offsets), ptr(x), ptr(_c(weight)), ptr(_c(bias)),
             ptr(_c(mean_scale)), float(eps), ptr(y), _stream(x.device))
        ctx.save_for_backward(x, weight, mean_scale, group_offsets)
        ctx.eps = eps
        return y

    @staticmethod
    def backward(ctx, g_y):
        x, weight, mean_scale, group_offsets = ctx.saved_tensors
        g_y = _c(g_y)
        G = group_offsets.numel() - 1
        D = x.shape[1]
        dev = x.device
        L = _lib.lib()
        gx = torch.empty_like(x)
        gw = torch.empty_like(weight)
        gb = torch.empty_like(weight)
        gms = torch.empty_like(weight)
        wp, wn = _lib.ws_ptr_size(L.mvml_graphnorm_bwd_workspace_size(G, D), dev)
        call("mvml_graphnorm_bwd", G, D, ptr(group_offsets), ptr(x), ptr(_c(weight)), ptr(_c(mean_scale)),
             float(ctx.eps), ptr(g_y), ptr(gx), ptr(gw), ptr(gb), ptr(gms), wp, wn, _stream(dev))
        return gx, gw, gb, gms, None, None


# linear_maxima's result: amx the int32 maxima tensor, slots [x, w, grad]; kx the (tensor, slot)
# holding max |x|; xrows x's per-row maxima (ROW_SCALES, else None); wil the weight's interleaved
# image (split_il4, may be None)
LinearMaxima = collections.namedtuple("LinearMaxima", "amx kx xrows wil")


def linear_maxima(x, w):
    """Split-fp16 maxima of a Linear's three products (LinearMaxima): x's from its producer when
    it folded one, one pass per operand instead of one per product, and (ROW_SCALES) x's per-row
    maxima for the forward product; None for the other algorithms."""
    if GEMM_ALGO != "f16x2":
        return None
    amx = zeros(3, dtype=torch.int32, device=x.device)
    M, K = x.shape
    xr = _row_scales(x, x, M, K, amx) if ROW_SCALES else None
    kx = (amx, 0) if ROW_SCALES else known_amax(x)
    if kx is None:
        absmax(x, M, K, K, amx, 0)
        kx = (amx, 0)
    return LinearMaxima(amx, kx, xr, _split_weight(w, amx))


def linear_fwd(x, weight, y, M, Nout, K, lm, bias=None, act=0, beta=0.0):
    """y = act(x W^T + b + beta y): the forward product of a Linear (per-row x scales when lm has
    them)."""
    if lm is not None and lm.xrows is not None:
        gemm(x, weight, M, Nout, K, 0, 0, K, K, y, Nout, bias=bias, act=act, beta=beta,
             amax=(None, slot(lm.amx, 1)), arows=lm.xrows, bil4=lm.wil)
    else:
        gemm(x, weight, M, Nout, K, 0, 0, K, K, y, Nout, bias=bias, act=act, beta=beta,
             amax=None if lm is None else (slot(*lm.kx), slot(lm.amx, 1)),
             bil4=None if lm is None else lm.wil)


def linear_dx(g, weight, gx, M, Nout, K, lm, beta=0.0):
    """gx = g W + beta gx (the data gradient of a Linear; per-row g scales under ROW_SCALES)."""
    if lm is not None and lm.xrows is not None:
        gemm(g, weight, M, K, Nout, 0, 1, Nout, K, gx, K, beta=beta, amax=(None, slot(lm.amx, 1)),
             arows=absmax_rows(g, M, Nout, Nout), bil4=lm.wil)
    else:
        gemm(g, weight, M, K, Nout, 0, 1, Nout, K, gx, K, beta=beta,
             amax=None if lm is None else (slot(lm.amx, 2), slot(lm.amx, 1)),
             bil4=None if lm is None else lm.wil)


def linear_forward(x, weight, bias, act=0, onto=None):
    """y = act(x W^T + b) of an nn.Linear (weight [out, in]; bias may be None) as one GEMM with
    a bias (+ ReLU, act 1) epilogue; onto: a contiguous [M, out] tensor the product is added to
    before bias and act (the GEMM's beta = 1), and which is then y.  Returns (x, weight, y, lm): the
    contiguous operands and the maxima record that linear_backward takes."""
    x = _c(x)
    M, K = x.shape
    Nout = weight.shape[0]
    y = torch.empty((M, Nout), dtype=torch.float32, device=x.device) if onto is None else onto
    weight = _c(weight)
    lm = linear_maxima(x, weight)
    linear_fwd(x, weight, y, M, Nout, K, lm, bias=None if bias is None else _c(bias), act=act,
               beta=0.0 if onto is None else 1.0)
    return x, weight, y, lm


def linear_backward(x, weight, g, lm, need_gb=True, need_gx=True, gx_acc=None):
    """(gx, gw, gb) of linear_forward from g, the contiguous gradient at its pre-activation:
    max |g| folded into lm's slot 2, gw = g^T x, gb = g's column sums, gx = g W (linear_dx);
    gb / gx None where not wanted.  gx_acc: a gradient x already has from another branch; gx is
    then that tensor with g W added by the product itself (beta = 1)."""
    M, K = x.shape
    Nout = weight.shape[0]
    if lm is not None:
        absmax(g, M, Nout, Nout, lm.amx, 2)
    gw = torch.empty_like(weight)
    gemm(g, x, Nout, K, M, 1, 1, Nout, K, gw, K,
         amax=None if lm is None else (slot(lm.amx, 2), slot(*lm.kx)))
    gb = None
    if need_gb:
        gb = torch.empty((Nout,), dtype=torch.float32, device=x.device)
        colsum(g, M, Nout, Nout, gb)
    gx = None
    if need_gx:
        gx = torch.empty_like(x) if gx_acc is None else gx_acc
        linear_dx(g, weight, gx, M, Nout, K, lm, beta=0.0 if gx_acc is None else 1.0)
    return gx, gw, gb


def dropout_seed():
    """A seed for mvml_dropout_fwd from torch's default (CPU) generator: reproducible under
    torch.manual_seed like nn.Dropout's draws, and no device round trip."""
    return int(torch.randint(0, 2 ** 62, (1,), dtype=torch.int64).item())


def dropout_p(module):
    """The probability an nn.Dropout module applies now (0 in eval mode)."""
    return float(module.p) if module.training and module.p > 0 else 0.0


def relu_dropout_(y, p):
    """nn.Dropout(p) in place on a ReLU output y (mvml_dropout_fwd); returns the backward's
    scale 1 / (1 - p) (1.0 for p == 0: nothing launched)."""
    if p <= 0.0:
        return 1.0
    if p >= 1.0:
        raise ValueError("dropout probability must be < 1 on the HIP path")
    call("mvml_dropout_fwd", y.numel(), ptr(y), ptr(y), float(p), dropout_seed(), _stream(y.device))
    return float(np.float32(1.0 / (1.0 - p)))  # the float the kernel multiplied by


class DropoutFunction(torch.autograd.Function):
    """nn.Dropout(p) anywhere (not only on a ReLU output, where a dropped element reads 0):
    mvml_dropout_fwd out of place with a seed from dropout_seed(); the backward is the same kernel
    on g_y with the saved (p, seed) — the mask is a function of (seed, element index) alone, so it
    is regenerated, not stored.  Use dropout() below: p == 0 (or eval mode) is the identity with
    no launch."""

    @staticmethod
    def forward(ctx, x, p, seed=None):
        _check_cuda_f32(x, "x")
        if p >= 1.0:
            raise ValueError("dropout probability must be < 1 on the HIP path")
        ctx.p = max(float(p), 0.0)
        if ctx.p == 0.0:  # the identity: nothing launched
            return x
        x = _c(x)
        ctx.seed = dropout_seed() if seed is None else int(seed)
        y = torch.empty_like(x)
        call("mvml_dropout_fwd", x.numel(), ptr(x), ptr(y), ctx.p, ctx.seed, _stream(x.device))
        return y

    @staticmethod
    def backward(ctx, g_y):
        if ctx.p == 0.0:
            return g_y, None, None
        g_y = _c(g_y)
        g_x = torch.empty_like(g_y)
        call("mvml_dropout_fwd", g_y.numel(), ptr(g_y), ptr(g_x), ctx.p, ctx.seed, _stream(g_y.device))
        return g_x, None, None


def dropout(x, p, seed=None):
    """nn.Dropout(p) in training mode on any float32 GPU tensor (DropoutFunction); p <= 0 returns
    x itself with nothing launched, p >= 1 is refused as in relu_dropout_."""
    if p >= 1.0:
        raise ValueError("dropout probability must be < 1 on the HIP path")
    if p <= 0.0:
        return x
    return DropoutFunction.apply(x, float(p), seed)


class BatchNorm1dFunction(torch.autograd.Function):
    """torch.nn.BatchNorm1d on (M, C) rows (csrc/batchnorm.hip).  Training mode normalises with
    the batch statistics and updates running_mean, running_var and num_batches_tracked inside
    the kernel; eval mode normalises with the running statistics.  fp64 statistics save_mean /
    save_invstd pass from the forward to the backward.  Under data parallelism the batch
    statistics are per rank, as torch's BatchNorm1d without SyncBatchNorm."""

    @staticmethod
    def forward(ctx, x, weight, bias, running_mean, running_var, num_batches_tracked, training, momentum, eps):
        _check_cuda_f32(x, "x")
        if x.dim() != 2:
            raise ValueError("BatchNorm1d: 2-D (M, C) inputs only on the HIP path")
        if momentum is None:
            raise ValueError("BatchNorm1d: momentum=None (cumulative average) is not implemented on the HIP path")
        if not training and (running_mean is None or running_var is None):
            raise ValueError("BatchNorm1d: eval mode needs running statistics")
        x = _rows_f32(x)
        M, C = x.shape
        dev = x.device
        if training and M == 1:
            raise ValueError(f"Expected more than 1 value per channel when training, got input size {tuple(x.shape)}")
        y = torch.empty((M, C), dtype=torch.float32, device=dev)
        save = torch.empty((2, C), dtype=torch.float64, device=dev)
        wp, wn = (None, 0)
        if training:
            wp, wn = _lib.ws_ptr_size(_lib.lib().mvml_batchnorm1d_workspace_size(M, C), dev)
        weight = None if weight is None else _c(weight)
        call("mvml_batchnorm1d_fwd", M, C, ptr(x), x.stride(0), ptr(weight), ptr(None if bias is None else _c(bias)),
             int(bool(training)), float(momentum), float(eps), ptr(running_mean), ptr(running_var),
             ptr(num_batches_tracked), ptr(y), C, ptr(save[0]), ptr(save[1]), wp, wn, _stream(dev))
        ctx.save_for_backward(x, weight, save)
        ctx.training = bool(training)
        return y

    @staticmethod
    def backward(ctx, g_y):
        x, weight, save = ctx.saved_tensors
        g_y = _rows_f32(g_y)
        M, C = x.shape
        dev = x.device
        g_x = torch.empty((M, C), dtype=torch.float32, device=dev) if ctx.needs_input_grad[0] else None
        g_w = torch.empty(C, dtype=torch.float32, device=dev) if weight is not None else None
        g_b = torch.empty(C, dtype=torch.float32, device=dev) if ctx.needs_input_grad[2] else None
        wp, wn = _lib.ws_ptr_size(_lib.lib().mvml_batchnorm1d_workspace_size(M, C), dev)
        call("mvml_batchnorm1d_bwd", M, C, ptr(x), x.stride(0), ptr(weight), int(ctx.training), ptr(save[0]),
             ptr(save[1]), ptr(g_y), g_y.stride(0), ptr(g_x), C, ptr(g_w), ptr(g_b), wp, wn, _stream(dev))
        return g_x, g_w, g_b, None, None, None, None, None, None


def batch_norm1d(x, bn):
    """x through the torch.nn.BatchNorm1d module `bn` (a parameter container: its weight, bias,
    buffers, eps, momentum and training flag are read; the arithmetic runs in the HIP kernels)."""
    if bn.momentum is None:
        raise ValueError("BatchNorm1d: momentum=None (cumulative average) is not implemented on the HIP path")
    training = bn.training or bn.running_mean is None
    return BatchNorm1dFunction.apply(x, bn.weight, bn.bias, bn.running_mean, bn.running_var,
                                     bn.num_batches_tracked if training else None, training, bn.momentum, bn.eps)


class LinearReLUFunction(torch.autograd.Function):
    """nn.Linear + nn.ReLU of GNNModule.fc (model.py:86-87) as one MFMA GEMM with a bias+ReLU
    epilogue, and the nn.Dropout(p) that follows it (model.py:87; p = 0: none) applied in place
    on the ReLU output: the backward then needs no mask (mvml_relu_bwd's scaled form)."""

    @staticmethod
    def forward(ctx, x, weight, bias, p=0.0):
        _check_cuda_f32(x, "x")
        x, weight, y, ctx.lm = linear_forward(x, weight, bias, act=1)
        if DEBUG_CAPTURE is not None:  # the ReLU sides the product took (parity tests)
            DEBUG_CAPTURE.setdefault("relu_out", []).append(y.detach().clone())
        ctx.scale = relu_dropout_(y, p)
        ctx.save_for_backward(x, weight, y)
        return y

    @staticmethod
    def backward(ctx, g_y):
        x, weight, y = ctx.saved_tensors
        g_y = _c(g_y)
        g_pre = torch.empty_like(y)
        call("mvml_relu_bwd", y.numel(), ptr(y), ptr(g_y), ptr(g_pre), float(ctx.scale), _stream(x.device))
        return (*linear_backward(x, weight, g_pre, ctx.lm, need_gx=ctx.needs_input_grad[0]), None)


def gatv2_fwd_bytes(N, E, H, F, out_cols, res_cols):
    """Algorithmic HBM bytes of one mvml_gatv2_agg_fwd (re-gathers of rows not counted, SURVEY.md
    §8d): read ZL, ZR and R once, rowptr, src ids, the attention vector; write out and attn."""
    return 4 * (2 * N * H * F + N * res_cols + N * out_cols + E * H + E + N + 1 + H * F)


def gatv2_bwd_bytes(N, E, H, F, out_cols, res_cols, mode):
    """Algorithmic bytes of mvml_gatv2_agg_bwd: read ZL, ZR, g_out (+ out for ELU'), attn, both
    CSRs; write gZL, gZR, gR, g_s (written, then read by source) and the g_attn partial rows."""
    P = int(_lib.lib().mvml_gatv2_partial_rows(N))
    return 4 * (4 * N * H * F + N * out_cols * (2 if mode == MODE_FLATTEN_ELU else 1) + N * res_cols
                + 3 * E * H + 2 * E + 2 * (N + 1) + 2 * P * H * F)


class GATv2LayerFunction(torch.autograd.Function):
    """dgllife GATv2Layer(GATv2Conv) forward / backward: one projection GEMM
    Y = X [W_src ; W_dst ; W_res]^T + [b_src | b_dst | b_res] (split-fp16 with per-row scales, the
    biases as its column bias), then mvml_gatv2_agg_fwd / mvml_gatv2_agg_bwd (csrc/gatv2_agg.hip).

    share_weights: w_dst and b_dst are None, Y has no W_dst block and ZR is ZL; the backward adds
    gZR onto gZL before the single block's products.  res_kind RES_PROJ: w_res (and b_res) ride in
    the GEMM, as their head mean in a head-mean layer (the layer only ever uses that);
    RES_IDENTITY: X, or its head mean, is R; RES_NONE: no R.  Parameters that do not exist get None
    gradients."""

    @staticmethod
    def forward(ctx, X, w_src, w_dst, w_res, b_src, b_dst, b_res, attn, g, H, F, slope, mode,
                res_kind=RES_PROJ):
        _check_res_kind("GATv2LayerFunction", res_kind, w_res)
        for t, n in ((X, "feat"), (w_src, "fc_src.weight"), (w_dst, "fc_dst.weight"), (w_res, "res_fc.weight"),
                     (b_src, "fc_src.bias"), (b_dst, "fc_dst.bias"), (b_res, "res_fc.bias"), (attn, "attn")):
            if t is not None:
                _check_cuda_f32(t, n)
        X, Xp = _padded_input(X)
        (N, Fin), Fp = X.shape, Xp.shape[1]
        dev = X.device
        st = _stream(dev)
        HF = H * F
        if res_kind == RES_IDENTITY and Fin != HF:
            raise ValueError(f"GATv2LayerFunction: the identity residual needs in_feats == H F ({Fin} != {HF})")
        mean = mode == MODE_MEAN
        shared = w_dst is None
        RW = F if mean else HF
        c_r = 0 if shared else HF               # ZR's column in Y / gZR's in gY
        c_res = HF if shared else 2 * HF        # the projected residual's
        C = c_res + (RW if res_kind == RES_PROJ else 0)
        # Wcat = [W_src ; W_dst ; W_res (head mean in a head-mean layer)], pad columns zero
        Wcat = torch.empty((C, Fp), dtype=torch.float32, device=dev)
        if Fp != Fin:
            zero_(Wcat)
        copy2d(Wcat[:HF, :Fin], _c(w_src))
        if not shared:
            copy2d(Wcat[HF:2 * HF, :Fin], _c(w_dst))
        biases = [b for b in (b_src, b_dst, b_res) if b is not None]
        bcat = zeros(C, device=dev) if biases else None
        if b_src is not None:
            copy2d(bcat[:HF], _c(b_src))
        if b_dst is not None:
            copy2d(bcat[HF:2 * HF], _c(b_dst))
        if res_kind == RES_PROJ:
            if mean:
                wm = torch.empty((F, Fin), dtype=torch.float32, device=dev)
                call("mvml_head_mean_f32", 1, H, F * Fin, ptr(_c(w_res)), HF * Fin, ptr(wm), F * Fin, st)
                copy2d(Wcat[c_res:, :Fin], wm)
                if b_res is not None:
                    bm = torch.empty(F, dtype=torch.float32, device=dev)
                    call("mvml_head_mean_f32", 1, H, F, ptr(_c(b_res)), HF, ptr(bm), F, st)
                    copy2d(bcat[c_res:], bm)
            else:
                copy2d(Wcat[c_res:, :Fin], _c(w_res))
                if b_res is not None:
                    copy2d(bcat[c_res:], _c(b_res))
        # split-fp16 maxima as GATLayerFunction's: every atom row at its own scale
        rows = GEMM_ALGO == "f16x2" and ROW_SCALES
        amx = xr = wil = None
        if rows:
            amx = zeros(3, dtype=torch.int32, device=dev)  # [X, Wcat, gY (bwd)]
            xr = _row_scales(X, Xp, N, Fp, amx)
            wil = _split_weight(Wcat, amx)
        ldy = _row_pitch(C)
        Y = torch.empty((N, ldy), dtype=torch.float32, device=dev)
        if rows:
            gemm(Xp, Wcat, N, C, Fp, 0, 0, Fp, Fp, Y, ldy, bias=bcat, amax=(None, slot(amx, 1)), arows=xr,
                 bil4=wil, role="gatv2_proj")
        else:
            gemm(Xp, Wcat, N, C, Fp, 0, 0, Fp, Fp, Y, ldy, bias=bcat, role="gatv2_proj")
        # the residual rows: Y's block (projected), the input or its head mean (identity), none
        R, ldr = None, 0
        if res_kind == RES_PROJ:
            R, ldr = Y[:, c_res:], ldy
        elif res_kind == RES_IDENTITY:
            R, ldr = _identity_residual(Xp, H, F, mean, st)
        out_cols = F if mean else HF
        E = g.num_edges()
        out = torch.empty((N, out_cols), dtype=torch.float32, device=dev)
        a = torch.empty((max(E, 1), H), dtype=torch.float32, device=dev)[:E]
        av = _c(attn).reshape(-1)
        _lib.call_tag[0] = {"layer": f"H{H}xF{F}",
                            "bytes": gatv2_fwd_bytes(N, E, H, F, out_cols, 0 if res_kind == RES_NONE else RW)}
        call("mvml_gatv2_agg_fwd", N, ptr(g.in_rowptr), ptr(g.in_src), ptr(Y), ldy, ptr(Y[:, c_r:]), ldy, H, F,
             ptr(av), ptr(R), ldr, float(slope), int(mode), ptr(out), ptr(a), st)
        if DEBUG_CAPTURE is not None:
            DEBUG_CAPTURE.setdefault("zlr_fwd", []).append(
                (Y[:, :HF].detach().clone(), Y[:, c_r:c_r + HF].detach().clone()))
        ctx.save_for_backward(Xp, Wcat, Y, a, out, av)
        ctx.mark_non_differentiable(a)
        ctx.g, ctx.H, ctx.F, ctx.slope, ctx.mode, ctx.Fin = g, H, F, slope, mode, Fin
        ctx.res_kind, ctx.shared = res_kind, shared
        ctx.has_b = (b_src is not None, b_dst is not None, b_res is not None)
        ctx.attn_shape = attn.shape
        ctx.amx, ctx.wil = amx, wil
        return out, a

    @staticmethod
    def backward(ctx, g_out, _g_a):
        Xp, Wcat, Y, a, out, av = ctx.saved_tensors
        g, H, F, mode, Fin = ctx.g, ctx.H, ctx.F, ctx.mode, ctx.Fin
        res_kind, shared, amx = ctx.res_kind, ctx.shared, ctx.amx
        g_out = _c(g_out)
        N, Fp = Xp.shape
        dev = Xp.device
        st = _stream(dev)
        HF = H * F
        mean = mode == MODE_MEAN
        RW = F if mean else HF
        c_r = 0 if shared else HF
        c_res = HF if shared else 2 * HF
        C, ldy = Wcat.shape[0], Y.shape[1]
        E = g.num_edges()
        L = _lib.lib()
        ldg = _row_pitch(C)
        gY = torch.empty((N, ldg), dtype=torch.float32, device=dev)
        # gZR: its own block of gY, or (share_weights) a buffer that is then added onto gZL
        gZR, ldgzr = (torch.empty((N, HF), dtype=torch.float32, device=dev), HF) if shared else (gY[:, HF:], ldg)
        # gR: gY's block (projected); the identity residual's share of dX written straight into gX
        # (flatten; a head-mean layer's is g_out itself: not formed); none otherwise
        gX = gR = None
        ldgr = 0
        if res_kind == RES_PROJ:
            gR, ldgr = gY[:, c_res:], ldg
        elif res_kind == RES_IDENTITY and not mean and ctx.needs_input_grad[0]:
            gX = torch.empty((N, Fin), dtype=torch.float32, device=dev)
            gR, ldgr = gX, Fin
        g_av = torch.empty(HF, dtype=torch.float32, device=dev)
        wp, wn = _lib.ws_ptr_size(L.mvml_gatv2_agg_bwd_workspace_size(N, E, H, F), dev)
        _lib.call_tag[0] = {"layer": f"H{H}xF{F}",
                            "bytes": gatv2_bwd_bytes(N, E, H, F, g_out.shape[1],
                                                     0 if res_kind == RES_NONE else RW, mode)}
        call("mvml_gatv2_agg_bwd", N, ptr(g.in_rowptr), ptr(g.in_src), ptr(g.out_rowptr), ptr(g.out_dst),
             ptr(g.out_inslot), E, ptr(Y), ldy, ptr(Y[:, c_r:]), ldy, H, F, ptr(av), ptr(a), ptr(out), ptr(g_out),
             float(ctx.slope), int(mode), ptr(gY), ldg, ptr(gZR), ldgzr, ptr(gR), ldgr, ptr(g_av), wp, wn, st)
        if shared:
            call("mvml_add_cols_f32", N, HF, ptr(gZR), ldgzr, ptr(gY), ldg, st)
        has_bs, has_bd, has_br = ctx.has_b
        f32 = dict(dtype=torch.float32, device=dev)
        g_bs = g_bd = g_br = None
        if has_bs:
            g_bs = torch.empty(HF, **f32)
            colsum(gY, N, HF, ldg, g_bs)
        if has_bd:
            g_bd = torch.empty(HF, **f32)
            colsum(gY, N, HF, ldg, g_bd, offset=HF)
        if has_br:
            g_br = torch.empty(HF, **f32)
            if mean:
                _head_mean_bias_grad(g_br, N, H, F, g_out, F)
            else:
                colsum(gY, N, HF, ldg, g_br, offset=c_res)
        # dL/dWcat = gY^T X and dL/dX = gY Wcat (+ the identity residual's share)
        if amx is not None:
            zero_(amx[2:3])
            absmax(gY, N, C, ldg, amx, 2)
        gW = torch.empty((C, Fp), **f32)
        gemm(gY, Xp, C, Fp, N, 1, 1, ldg, Fp, gW, Fp,
             amax=None if amx is None else (slot(amx, 2), slot(amx, 0)), role="gatv2_dw")
        g_ws = copy2d(torch.empty((HF, Fin), **f32), gW[:HF, :Fin])
        g_wd = None if shared else copy2d(torch.empty((HF, Fin), **f32), gW[HF:2 * HF, :Fin])
        g_wr = None
        if res_kind == RES_PROJ:
            g_wr = torch.empty((HF, Fin), **f32)
            if mean:
                gm = copy2d(torch.empty((F, Fin), **f32), gW[c_res:, :Fin])
                call("mvml_head_mean_bwd_f32", 1, H, F * Fin, ptr(gm), F * Fin, ptr(g_wr), HF * Fin, st)
            else:
                copy2d(g_wr, gW[c_res:, :Fin])
        if ctx.needs_input_grad[0]:
            beta = 1.0 if res_kind == RES_IDENTITY else 0.0
            if gX is None:
                gX = _new_gx(g_out, N, Fin, H, F, res_kind == RES_IDENTITY, st)
            if amx is not None:
                gemm(gY, Wcat, N, Fin, C, 0, 1, ldg, Fp, gX, Fin, amax=(None, slot(amx, 1)),
                     arows=absmax_rows(gY, N, C, ldg), bil4=ctx.wil, beta=beta)
            else:
                gemm(gY, Wcat, N, Fin, C, 0, 1, ldg, Fp, gX, Fin, beta=beta)
        else:
            gX = None
        return (gX, g_ws, g_wd, g_wr, g_bs, g_bd, g_br, g_av.view(ctx.attn_shape),
                None, None, None, None, None, None)


# ---- GCN (dgl 0.9.1 GraphConv; csrc/gcn_agg.hip) ------------------------------------------------
GCN_NORMS = {"none": 0, "both": 1, "right": 2, "left": 3}


def gcn_agg_bytes(N, E, D):
    """Algorithmic HBM bytes of one mvml_gcn_agg: read X and write out once, the row pointers, the
    neighbour ids and the two scale vectors (re-gathers of rows not counted)."""
    return 4 * (2 * N * D + N + 1 + E + 2 * N)


def gcn_scales(g, norm):
    """(src_scale, dst_scale) of GraphConv's `norm` on the device batch g (mvml_gcn_norm_scales),
    None where the factor is 1 for every atom.  Computed once per (graph, norm) and kept on the
    batch; BatchedMolGraph.recollate() drops them with the indices it rebuilds."""
    if norm not in GCN_NORMS:
        raise ValueError(f'Invalid norm value. Must be either "none", "both", "right" or "left". But got "{norm}".')
    if norm == "none":
        return None, None
    cache = g._dev.setdefault("gcn_scales", {})
    if norm not in cache:
        N = g.num_nodes()
        s = torch.empty((2, max(N, 1)), dtype=torch.float32, device=g.device)
        call("mvml_gcn_norm_scales", N, ptr(g.in_rowptr), ptr(g.out_rowptr), GCN_NORMS[norm], ptr(s[0]), ptr(s[1]),
             _stream(g.device))
        cache[norm] = (s[0] if norm != "right" else None, s[1] if norm != "left" else None)
    return cache[norm]


def gcn_agg(X, ldx, D, g, scales, transpose=False, bias=None, act=0, rows=False):
    """mvml_gcn_agg of the [N, D] rows of X (row stride ldx) over g's in-CSR, or (transpose) the
    adjoint over its out-CSR with the two scales swapped; a new dense [N, D] tensor, with its
    per-row maxima recorded on it (fold_rows) when `rows`."""
    N, E = g.num_nodes(), g.num_edges()
    dev = X.device
    out = torch.empty((N, D), dtype=torch.float32, device=dev)
    rmx = torch.empty(max(N, 1), dtype=torch.int32, device=dev) if rows else None
    src_scale, dst_scale = scales
    rowptr, nbr = (g.out_rowptr, g.out_dst) if transpose else (g.in_rowptr, g.in_src)
    nbr_scale, row_scale = (dst_scale, src_scale) if transpose else (src_scale, dst_scale)
    _lib.call_tag[0] = {"layer": f"D{D}", "bytes": gcn_agg_bytes(N, E, D)}
    call("mvml_gcn_agg", N, ptr(rowptr), ptr(nbr), ptr(X), ldx, D, ptr(nbr_scale), ptr(row_scale), ptr(bias),
         int(act), ptr(out), D, None, ptr(rmx), _stream(dev))
    if rows:
        fold_rows(out, rmx)
    return out


def _graph_conv_forward(X, weight, bias, g, norm, act):
    """GraphConv's forward.  Returns (out, (A, Wp), state): A the product's [N, Fp] operand (the
    zero-padded input, or the aggregated input), Wp the [Fp, out] weight it met, state what the
    backward needs beside them and `out`."""
    for t, n in ((X, "feat"), (weight, "weight"), (bias, "bias")):
        if t is not None:
            _check_cuda_f32(t, n)
    Xpad = zero_padded(X, _round4(X.shape[1])) if X.dim() == 2 else None
    if Xpad is None:
        X = _c(X)
    N, Fin = X.shape
    Fout = weight.shape[1]
    dev = X.device
    Fp = _round4(Fin)
    weight = _c(weight)
    bias = None if bias is None else _c(bias)
    scales = gcn_scales(g, norm)
    proj_first = Fin > Fout or Fin != Fp
    rows = GEMM_ALGO == "f16x2" and ROW_SCALES
    amx = zeros(3, dtype=torch.int32, device=dev) if rows else None  # [A operand, W, gradient]
    if proj_first:
        # operands of the product padded to 16-B rows / a K of 4 q (zeros add nothing)
        Xp, Wp = Xpad if Xpad is not None else X, weight
        if Xpad is None and Fp != Fin:
            Xp = zeros((N, Fp), device=dev)
            copy2d(Xp[:, :Fin], X)
        if Fp != Fin:
            Wp = zeros((Fp, Fout), device=dev)
            copy2d(Wp[:Fin], weight)
        A = Xp
    else:
        Wp = weight
        A = gcn_agg(X, Fin, Fin, g, scales, rows=rows)
    xr = None
    if rows:
        xr = _row_scales(X if proj_first else A, A, N, Fp, amx)
        absmax(Wp, Fp, Fout, Fout, amx, 1)
    last_gemm = not proj_first
    Y = torch.empty((N, Fout), dtype=torch.float32, device=dev)
    gemm(A, Wp, N, Fout, Fp, 0, 1, Fp, Fout, Y, Fout, bias=bias if last_gemm else None,
         act=act if last_gemm else 0, amax=(None, slot(amx, 1)) if rows else None, arows=xr, role="gcn_proj")
    out = Y if last_gemm else gcn_agg(Y, Fout, Fout, g, scales, bias=bias, act=act, rows=rows)
    if DEBUG_CAPTURE is not None and act:  # the ReLU sides the product took (parity tests)
        DEBUG_CAPTURE.setdefault("gcn_out", []).append(out.detach().clone())
    return out, (A, Wp), (g, scales, proj_first, Fin, amx, bias is not None)


def _graph_conv_backward(A, Wp, out, state, g_out, need_gx, gx_acc=None):
    """(gX, gW, gb) of GraphConv from g_out; out: the saved output of a ReLU layer, else None.
    gx_acc: an [N, in_feats] gradient the input already has from another branch (GCNLayer's
    residual), accumulated onto with the data-gradient product's beta = 1 or mvml_add_cols_f32,
    so that no framework add runs."""
    g, scales, proj_first, Fin, amx, has_bias = state
    N, Fp = A.shape
    Fout = Wp.shape[1]
    dev = A.device
    g_out = _c(g_out)
    if out is not None:
        g_pre = torch.empty_like(g_out)
        call("mvml_relu_bwd", g_out.numel(), ptr(out), ptr(g_out), ptr(g_pre), 1.0, _stream(dev))
    else:
        g_pre = g_out
    gb = None
    if has_bias:
        gb = torch.empty(Fout, dtype=torch.float32, device=dev)
        colsum(g_pre, N, Fout, Fout, gb)
    rows = amx is not None
    # the gradient at the product's output: through the sum's adjoint when the sum came last
    gY = gcn_agg(g_pre, Fout, Fout, g, scales, transpose=True, rows=rows) if proj_first else g_pre
    gyr = _row_scales(gY, gY, N, Fout, amx, 2) if rows else None
    gW = torch.empty((Fp, Fout), dtype=torch.float32, device=dev)
    gemm(A, gY, Fp, Fout, N, 1, 1, Fp, Fout, gW, Fout,
         amax=(slot(amx, 0), slot(amx, 2)) if rows else None, role="gcn_dw")
    gX = None
    if need_gx:
        into = proj_first and gx_acc is not None  # the product writes dX itself: accumulate there
        gA = gx_acc if into else torch.empty((N, Fin), dtype=torch.float32, device=dev)
        gemm(gY, Wp, N, Fin, Fout, 0, 0, Fout, Fout, gA, Fin, beta=1.0 if into else 0.0,
             amax=(None, slot(amx, 1)) if rows else None, arows=gyr, role="gcn_dx")
        gX = gA
        if not proj_first:
            gX = gcn_agg(gA, Fin, Fin, g, scales, transpose=True)
            if gx_acc is not None:  # (in_feats % 4 == 0 in this order)
                call("mvml_add_cols_f32", N, Fin, ptr(gx_acc), Fin, ptr(gX), Fin, _stream(dev))
    return gX, gW[:Fin], gb


class GraphConvFunction(torch.autograd.Function):
    """dgl 0.9.1 GraphConv.forward (restated; parity with dgl is unpinned):
    act(D_dst (A (D_src X)) W + b), the sum over in-edges on mvml_gcn_agg and the product on the
    fp32-accurate GEMM with the [in, out] weight read K-major (no transposed copy).  The sum runs
    on the narrower side as in DGL (the product first when in_feats > out_feats), and on the
    projected side whenever in_feats is no multiple of 4 (the aggregation's float4 rows; the two
    orders are the same function).  Bias and ReLU ride in whichever launch comes last.  Backward:
    mvml_relu_bwd on the saved output, the aggregation over the out-CSR with the scales swapped
    (a gather: no atomics), the split-K weight-gradient product and mvml_colsum_f32."""

    @staticmethod
    def forward(ctx, X, weight, bias, g, norm, act):
        out, (A, Wp), ctx.state = _graph_conv_forward(X, weight, bias, g, norm, act)
        ctx.save_for_backward(A, Wp, out if act else None)
        return out

    @staticmethod
    def backward(ctx, g_out):
        A, Wp, out = ctx.saved_tensors
        gX, gW, gb = _graph_conv_backward(A, Wp, out, ctx.state, g_out, ctx.needs_input_grad[0])
        return gX, gW, gb, None, None, None


class GCNConvResidualFunction(torch.autograd.Function):
    """dgllife GCNLayer up to its Dropout: graph_conv(g, x) + act(res_connection(x)), act ReLU or
    none on both branches, as ONE autograd node.  The input feeds both branches; as two Functions
    the autograd engine would add their two input gradients with a framework kernel, so the
    backward here forms the residual Linear's dX first and the conv's data gradient accumulates
    onto it (_graph_conv_backward's gx_acc).  The sum goes to a new tensor (mvml_copy_cols, then
    mvml_add_cols_f32): both branch outputs are kept for their ReLU backwards."""

    @staticmethod
    def forward(ctx, X, weight, bias, res_w, res_b, g, norm, act):
        conv, (A, Wp), ctx.state = _graph_conv_forward(X, weight, bias, g, norm, act)
        _check_cuda_f32(res_w, "res_connection.weight")
        x, res_w, y, ctx.lm = linear_forward(X, res_w, res_b, act=int(act))
        if DEBUG_CAPTURE is not None and act:
            DEBUG_CAPTURE.setdefault("relu_out", []).append(y.detach().clone())
        s = copy2d(torch.empty_like(conv), conv)
        M, Fout = y.shape
        if M:
            call("mvml_add_cols_f32", M, Fout, ptr(y), Fout, ptr(s), Fout, _stream(x.device))
        ctx.save_for_backward(A, Wp, conv if act else None, x, res_w, y if act else None)
        ctx.has_res_b = res_b is not None
        return s

    @staticmethod
    def backward(ctx, g_s):
        A, Wp, conv, x, res_w, y = ctx.saved_tensors
        g_s = _c(g_s)
        if y is not None:
            g_pre = torch.empty_like(g_s)
            call("mvml_relu_bwd", g_s.numel(), ptr(y), ptr(g_s), ptr(g_pre), 1.0, _stream(x.device))
        else:
            g_pre = g_s
        need = ctx.needs_input_grad[0]
        gx, g_rw, g_rb = linear_backward(x, res_w, g_pre, ctx.lm, need_gb=ctx.has_res_b, need_gx=need)
        gX, gW, gb = _graph_conv_backward(A, Wp, conv, ctx.state, g_s, need, gx_acc=gx)
        return gX, gW, gb, g_rw, g_rb, None, None, None


# ---- GraphSAGE (dgl 0.9.1 SAGEConv; csrc/sage_agg.hip) ------------------------------------------
SAGE_AGGREGATORS = ("mean", "gcn", "pool")


def sage_max_fwd_bytes(N, E, D):
    """Algorithmic HBM bytes of one mvml_sage_max_fwd: read X, write out and arg once, the row
    pointers and the neighbour ids (gcn_agg_bytes without the scale vectors, plus the arg row)."""
    return 4 * (3 * N * D + N + 1 + E)


def sage_max_bwd_bytes(N, E, D, gated):
    """Algorithmic bytes of one mvml_sage_max_bwd: read G and arg (and the gate P) once, write gX,
    the row pointers, the destination ids and the in-slots."""
    return 4 * ((3 + int(bool(gated))) * N * D + N + 1 + 2 * E)


def sage_gcn_scale(g):
    """1 / (in_degree + 1) per atom of the device batch g (mvml_sage_gcn_scale), computed once and
    kept on the batch as gcn_scales' factors are; BatchedMolGraph.recollate() drops it."""
    s = g._dev.get("sage_gcn_scale")
    if s is None:
        N = g.num_nodes()
        s = g._dev["sage_gcn_scale"] = torch.empty(max(N, 1), dtype=torch.float32, device=g.device)
        call("mvml_sage_gcn_scale", N, ptr(g.in_rowptr), ptr(s), _stream(g.device))
    return s


def sage_max(X, ldx, D, g, rows=False):
    """(out, arg) of mvml_sage_max_fwd on the [N, D] rows of X (row stride ldx) over g's in-CSR: new
    dense [N, D] tensors, out's per-row maxima recorded on it (fold_rows) when `rows`."""
    N, E = g.num_nodes(), g.num_edges()
    dev = X.device
    out = torch.empty((N, D), dtype=torch.float32, device=dev)
    arg = torch.empty((N, D), dtype=torch.int32, device=dev)
    rmx = torch.empty(max(N, 1), dtype=torch.int32, device=dev) if rows else None
    _lib.call_tag[0] = {"layer": f"D{D}", "bytes": sage_max_fwd_bytes(N, E, D)}
    call("mvml_sage_max_fwd", N, ptr(g.in_rowptr), ptr(g.in_src), ptr(X), ldx, D, ptr(out), D, ptr(arg), D, None,
         ptr(rmx), _stream(dev))
    if rows:
        fold_rows(out, rmx)
    return out, arg


def sage_max_grad(G, arg, D, g, gate=None):
    """mvml_sage_max_bwd: the [N, D] gradient of sage_max's input from G, the gradient at its
    output, gathered over g's out-CSR at the saved arg; gate: the pooled ReLU output, whose
    backward rides in the same pass."""
    N, E = g.num_nodes(), g.num_edges()
    gX = torch.empty((N, D), dtype=torch.float32, device=G.device)
    _lib.call_tag[0] = {"layer": f"D{D}", "bytes": sage_max_bwd_bytes(N, E, D, gate is not None)}
    call("mvml_sage_max_bwd", N, ptr(g.out_rowptr), ptr(g.out_dst), ptr(g.out_inslot), ptr(G), D, ptr(arg), D, D,
         ptr(gate), D, ptr(gX), D, _stream(G.device))
    return gX


def sage_self_add(X, scale, out, bias=None, act=0):
    """out = act(scale[:, None] * X + out + bias) in place on the dense [N, D] out (mvml_sage_self_add)."""
    N, D = out.shape
    call("mvml_sage_self_add", N, ptr(X), D, D, ptr(scale), ptr(bias), int(act), ptr(out), D, _stream(out.device))
    return out


def _share_rows(x, lm):
    """Leave the per-row maxima that one Linear's forward took of x on x, for the next Linear
    that reads the same tensor."""
    if lm is not None and lm.xrows is not None and known_rows(x) is None:
        fold_rows(x, lm.xrows)


class SAGEConvFunction(torch.autograd.Function):
    """dgl 0.9.1 SAGEConv.forward after feat_drop (restated; parity with dgl is unpinned), as ONE
    autograd node:
      mean: act(fc_self(x) + fc_neigh(mean_in x) + b)       (mvml_gcn_agg, norm "right")
      gcn:  act(fc_neigh((sum_in x + x) / (deg + 1)) + b)   (mvml_gcn_agg, mvml_sage_self_add)
      pool: act(fc_self(x) + fc_neigh(max_in relu(fc_pool(x))) + b)   (mvml_sage_max_fwd)
    mean and gcn apply fc_neigh before the aggregation when in_feats > out_feats, as DGL does, and
    whenever in_feats is no multiple of 4 (the aggregation's float4 rows; the same function); pool
    runs its in_feats-wide middle zero-padded to a multiple of 4.  The products are nn.Linear
    products on the fp32-accurate GEMM; the second branch's product adds onto the first's output
    (beta = 1) with bias and ReLU in its epilogue, so no separate add runs.  Backward: the input
    feeds fc_self and the neighbour branch (and fc_pool); the later data-gradient product
    accumulates onto the earlier one (beta = 1), so the autograd engine adds nothing.  The
    maximum's backward is a gather at the saved arg with fc_pool's ReLU folded in."""

    @staticmethod
    def forward(ctx, X, w_pool, b_pool, w_self, w_neigh, bias, g, aggr, act):
        for t, n in ((X, "feat"), (w_pool, "fc_pool.weight"), (b_pool, "fc_pool.bias"), (w_self, "fc_self.weight"),
                     (w_neigh, "fc_neigh.weight"), (bias, "bias")):
            if t is not None:
                _check_cuda_f32(t, n)
        if aggr not in SAGE_AGGREGATORS:
            raise KeyError(f"Aggregator type {aggr} not recognized.")
        N, Fin = X.shape
        Fout = w_neigh.shape[0]
        Fp = _round4(Fin)
        dev = X.device
        bias = None if bias is None else _c(bias)
        rows = GEMM_ALGO == "f16x2" and ROW_SCALES
        proj_first = aggr != "pool" and (Fin > Fout or Fp != Fin)
        P = M = arg = A = lm_p = lm_s = wp = ws = None
        if aggr == "pool":
            wp, bp, wn = w_pool, b_pool, w_neigh
            if Fp != Fin:  # the pooled rows and fc_neigh's K zero-padded to float4 rows (zeros add nothing)
                wp = zeros((Fp, Fin), device=dev)
                copy2d(wp[:Fin], _c(w_pool))
                bp = zeros(Fp, device=dev)
                copy2d(bp[:Fin], _c(b_pool))
                wn = zeros((Fout, Fp), device=dev)
                copy2d(wn[:, :Fin], _c(w_neigh))
            x, wp, P, lm_p = linear_forward(X, wp, bp, act=1)
            _share_rows(x, lm_p)
            M, arg = sage_max(P, Fp, Fp, g, rows=rows)
            _, ws, out, lm_s = linear_forward(x, w_self, None)
            _, wn, out, lm_n = linear_forward(M, wn, bias, act=act, onto=out)
            if DEBUG_CAPTURE is not None:  # fc_pool's ReLU sides and the maximum's ties (parity tests)
                DEBUG_CAPTURE.setdefault("sage_pool", []).append(P.detach().clone())
                DEBUG_CAPTURE.setdefault("sage_arg", []).append(arg.detach().clone())
        elif aggr == "mean":
            scales = gcn_scales(g, "right")
            if proj_first:
                x, wn, Y, lm_n = linear_forward(X, w_neigh, None)
                _share_rows(x, lm_n)
                H = gcn_agg(Y, Fout, Fout, g, scales)
                _, ws, out, lm_s = linear_forward(x, w_self, bias, act=act, onto=H)
            else:
                x = _c(X)
                A = gcn_agg(x, Fin, Fin, g, scales, rows=rows)
                _, ws, out, lm_s = linear_forward(x, w_self, None)
                _, wn, out, lm_n = linear_forward(A, w_neigh, bias, act=act, onto=out)
        else:
            s = sage_gcn_scale(g)
            if proj_first:
                x, wn, Y, lm_n = linear_forward(X, w_neigh, None)
                out = gcn_agg(Y, Fout, Fout, g, (None, s))
                sage_self_add(Y, s, out, bias, act)
            else:
                x = _c(X)
                A = gcn_agg(x, Fin, Fin, g, (None, s))
                sage_self_add(x, s, A)
                _, wn, out, lm_n = linear_forward(A, w_neigh, bias, act=act)
        if DEBUG_CAPTURE is not None and act:  # the ReLU sides the product took (parity tests)
            DEBUG_CAPTURE.setdefault("sage_out", []).append(out.detach().clone())
        ctx.save_for_backward(x, wp, ws, wn, P, M, arg, A, out if act else None)
        ctx.state = (g, aggr, proj_first, Fin, Fout, Fp, lm_p, lm_s, lm_n, bias is not None)
        return out

    @staticmethod
    def backward(ctx, g_out):
        x, wp, ws, wn, P, M, arg, A, out = ctx.saved_tensors
        g, aggr, proj_first, Fin, Fout, Fp, lm_p, lm_s, lm_n, has_bias = ctx.state
        N = x.shape[0]
        dev = x.device
        need = ctx.needs_input_grad[0]
        g_out = _c(g_out)
        if out is not None:
            g_pre = torch.empty_like(g_out)
            call("mvml_relu_bwd", g_out.numel(), ptr(out), ptr(g_out), ptr(g_pre), 1.0, _stream(dev))
        else:
            g_pre = g_out
        gb = None
        if has_bias:
            gb = torch.empty(Fout, dtype=torch.float32, device=dev)
            colsum(g_pre, N, Fout, Fout, gb)
        gX = gWp = gbp = gWs = None
        if aggr == "pool":
            gM, gWn, _ = linear_backward(M, wn, g_pre, lm_n, need_gb=False)
            gP = sage_max_grad(gM, arg, Fp, g, gate=P)
            gX, gWp, gbp = linear_backward(x, wp, gP, lm_p, need_gx=need)
            gX, gWs, _ = linear_backward(x, ws, g_pre, lm_s, need_gb=False, need_gx=need, gx_acc=gX)
            if Fp != Fin:
                gWp, gbp = gWp[:Fin], gbp[:Fin]
                gWn = copy2d(torch.empty((Fout, Fin), dtype=torch.float32, device=dev), gWn[:, :Fin])
        elif aggr == "mean":
            scales = gcn_scales(g, "right")
            if proj_first:
                gX, gWs, _ = linear_backward(x, ws, g_pre, lm_s, need_gb=False, need_gx=need)
                gY = gcn_agg(g_pre, Fout, Fout, g, scales, transpose=True)
                gX, gWn, _ = linear_backward(x, wn, gY, lm_n, need_gb=False, need_gx=need, gx_acc=gX)
            else:
                gA, gWn, _ = linear_backward(A, wn, g_pre, lm_n, need_gb=False, need_gx=need)
                if need:
                    gX = gcn_agg(gA, Fin, Fin, g, scales, transpose=True)
                _, gWs, _ = linear_backward(x, ws, g_pre, lm_s, need_gb=False, need_gx=need, gx_acc=gX)
        else:
            s = sage_gcn_scale(g)
            if proj_first:
                gY = gcn_agg(g_pre, Fout, Fout, g, (None, s), transpose=True)
                sage_self_add(g_pre, s, gY)
                gX, gWn, _ = linear_backward(x, wn, gY, lm_n, need_gb=False, need_gx=need)
            else:
                gA, gWn, _ = linear_backward(A, wn, g_pre, lm_n, need_gb=False, need_gx=need)
                if need:
                    gX = gcn_agg(gA, Fin, Fin, g, (None, s), transpose=True)
                    sage_self_add(gA, s, gX)
        return gX, gWp, gbp, gWs, gWn, gb, None, None, None


# ---- GIN with bond embeddings (dgllife 0.3.0 gnn/gin.py; csrc/gin_agg.hip, csrc/segment_pool.hip) ----
GIN_MAX_TABLES = 4       # embedding tables per side (mvml_gin_edge_codes, mvml_embed_sum_fwd)
GIN_MAX_EDGE_ROWS = 256  # rows over all edge tables: one byte per table in a slot's code
EMBED_MAX_ROWS = 128     # rows of one node table
POOL_MODES = {"sum": 0, "mean": 1, "max": 2}


def gin_agg_fwd_bytes(N, E, D, R):
    """Algorithmic HBM bytes of one mvml_gin_agg_fwd: read X and write out once, the row pointers,
    the neighbour ids, one code per slot and the R table rows (re-gathers of rows not counted)."""
    return 4 * (2 * N * D + N + 1 + 2 * E + R * D)


def gin_edge_emb_grad_bytes(N, E, D, R):
    """Algorithmic bytes of one mvml_gin_edge_emb_grad: read G once, the row pointers and the codes;
    write and re-read the mvml_gin_partial_rows(N) partial tables, write dE."""
    P = _lib.lib().mvml_gin_partial_rows(N)
    return 4 * (N * D + N + 1 + E + 2 * P * R * D + R * D)


def embed_sum_fwd_bytes(N, T, D, R):
    """Algorithmic bytes of one mvml_embed_sum_fwd: T indices per atom, the R table rows, out."""
    return 4 * (N * T + R * D + N * D)


def embed_sum_bwd_bytes(N, T, D, R):
    """Algorithmic bytes of one mvml_embed_sum_bwd: G once, T indices per atom, the partial tables
    written and re-read, dTab."""
    P = _lib.lib().mvml_gin_partial_rows(N)
    return 4 * (N * D + N * T + 2 * P * R * D + R * D)


def segment_pool_bytes(B, N, D, mode):
    """Algorithmic bytes of one mvml_segment_pool_fwd or _bwd: the [N, D] rows once, the [B, D]
    rows once (twice with max's argmax), the offsets."""
    return 4 * (N * D + (2 if POOL_MODES[mode] == 2 else 1) * B * D) + 8 * (B + 1)


def _index_tensors(cats, n, dev, what):
    """The T category tensors of one side as int32 device vectors of length n."""
    cats = list(cats)
    if not 1 <= len(cats) <= GIN_MAX_TABLES:
        raise ValueError(f"{what}: 1 to {GIN_MAX_TABLES} categorical feature tensors, got {len(cats)}")
    out = []
    for c in cats:
        if not c.is_cuda:
            raise RuntimeError(f"{what} must be CUDA (HIP) tensors: the mvml_gat path has no CPU fallback")
        if c.dim() != 1 or c.shape[0] != n or c.dtype.is_floating_point:
            raise ValueError(f"{what}: integer vectors of length {n} expected, got {tuple(c.shape)} {c.dtype}")
        out.append(_c(c if c.dtype == torch.int32 else c.to(torch.int32)))
    return out


def _table_args(cats, sizes):
    """(T, four pointers, four sizes) of an entry point that takes up to four tables."""
    T = len(sizes)
    ps = [ptr(c) for c in cats] + [None] * (GIN_MAX_TABLES - T)
    ns = [int(s) for s in sizes] + [0] * (GIN_MAX_TABLES - T)
    return (T, *ps, *ns)


def concat_tables(tables):
    """The embedding tables [n_t, D] as one [R, D] tensor (mvml_copy_cols per table), and R."""
    D = tables[0].shape[1]
    R = sum(t.shape[0] for t in tables)
    tab = torch.empty((R, D), dtype=torch.float32, device=tables[0].device)
    o = 0
    for t in tables:
        copy2d(tab[o:o + t.shape[0]], _c(t))
        o += t.shape[0]
    return tab, R


def _split_rows(dtab, tables):
    """The per-table row blocks of a dense [R, D] gradient (contiguous views)."""
    out, o = [], 0
    for t in tables:
        out.append(dtab[o:o + t.shape[0]])
        o += t.shape[0]
    return out


def gin_edge_codes(g, edge_feats, sizes):
    """One int32 per in-CSR slot of the device batch g holding, in byte t, the row of the slot's
    edge in the concatenated edge tables (mvml_gin_edge_codes).  Computed once per (batch, feature
    tensors, table sizes) and kept on the batch as gcn_scales' factors are;
    BatchedMolGraph.recollate() drops it.  Categories outside their table raise IndexError, as
    nn.Embedding would (one host read per batch, when the codes are first made)."""
    sizes = tuple(int(s) for s in sizes)
    E = g.num_edges()
    feats = list(edge_feats)
    if len(feats) != len(sizes):
        raise ValueError(f"{len(sizes)} edge tables but {len(feats)} categorical edge feature tensors")
    # keyed by the tensors given (not by their int32 copies, which are made on a miss only)
    key = (sizes, tuple(c.data_ptr() for c in feats), tuple(c._version for c in feats))
    cache = g._dev.setdefault("gin_codes", {})
    if key not in cache:
        cats = _index_tensors(feats, E, g.device, "categorical_edge_feats")
        codes = torch.empty(max(E, 1), dtype=torch.int32, device=g.device)
        status = zeros(1, dtype=torch.int32, device=g.device)
        call("mvml_gin_edge_codes", E, *_table_args(cats, sizes), ptr(g.in_eid), ptr(codes), ptr(status),
             _stream(g.device))
        bad = int(status.item())
        if bad:
            raise IndexError(f"{bad} categorical edge features lie outside their embedding tables {sizes}")
        cache[key] = (codes, feats)  # (the given tensors are kept: their addresses are the key)
    return cache[key][0]


def gin_agg(X, D, g, codes, tab, R, T, rows=False):
    """mvml_gin_agg_fwd of the dense [N, D] rows of X over g's in-CSR with the concatenated edge
    tables tab [R, D]: a new dense [N, D] tensor, its per-row maxima recorded on it when `rows`."""
    N, E = g.num_nodes(), g.num_edges()
    dev = X.device
    out = torch.empty((N, D), dtype=torch.float32, device=dev)
    rmx = torch.empty(max(N, 1), dtype=torch.int32, device=dev) if rows else None
    _lib.call_tag[0] = {"layer": f"D{D}", "bytes": gin_agg_fwd_bytes(N, E, D, R)}
    call("mvml_gin_agg_fwd", N, ptr(g.in_rowptr), ptr(g.in_src), ptr(codes), ptr(X), X.stride(0), D, ptr(tab), D,
         R, T, ptr(out), D, None, ptr(rmx), _stream(dev))
    if rows:
        fold_rows(out, rmx)
    return out


def _emb_grad_ws(N, R, D, dev):
    return _lib.ws_ptr_size(_lib.lib().mvml_gin_emb_grad_workspace_size(N, R, D), dev)


def gin_edge_emb_grad(G, D, g, codes, R, T):
    """mvml_gin_edge_emb_grad: the dense [R, D] gradient of the concatenated edge tables from G,
    the gradient at gin_agg's output."""
    N, E = g.num_nodes(), g.num_edges()
    dE = torch.empty((R, D), dtype=torch.float32, device=G.device)
    wp, wn = _emb_grad_ws(N, R, D, G.device)
    _lib.call_tag[0] = {"layer": f"D{D}", "bytes": gin_edge_emb_grad_bytes(N, E, D, R)}
    call("mvml_gin_edge_emb_grad", N, ptr(g.in_rowptr), ptr(codes), ptr(G), G.stride(0), D, R, T, ptr(dE), wp, wn,
         _stream(G.device))
    return dE


class _StageCtx:
    """A stand-in ctx for running another Function's forward / backward as a stage of a fused one."""

    def __init__(self, needs=(True,) * 9):
        self.needs_input_grad = needs
        self.saved_tensors = ()

    def save_for_backward(self, *ts):
        self.saved_tensors = ts


class GINLayerFunction(torch.autograd.Function):
    """dgllife 0.3.0 GINLayer.forward (restated; parity with dgllife is unpinned) as ONE autograd
    node: the slot codes of the bond categories (gin_edge_codes, cached on the batch) -> the fused
    sum over in-edges of (node_feats[u] + e_uv) with e_uv the sum of the edge's embedding rows
    (mvml_gin_agg_fwd) -> mlp = Linear(D, 2D) + ReLU -> Linear(2D, D) on the fp32-accurate GEMM ->
    BatchNorm1d (bn: the parameter container, or None) -> ReLU (act; mvml_relu_f32 in place) and
    the Dropout(p) that follows a ReLU layer (in place, relu_dropout_).  Backward: mvml_relu_bwd,
    the BatchNorm backward, the two Linears' backwards, then from the gradient at the sum's output
    both the edge tables' gradient (mvml_gin_edge_emb_grad) and the input's (mvml_gcn_agg over the
    out-CSR).  Returns gradients for X, both Linears, BatchNorm and every edge table."""

    @staticmethod
    def forward(ctx, X, w1, b1, w2, b2, bn_w, bn_b, g, edge_feats, bn, act, p, *tables):
        _check_cuda_f32(X, "node_feats")
        for t in (w1, b1, w2, b2, *tables):
            _check_cuda_f32(t, "GINLayer parameters")
        X = _rows_f32(X)
        N, D = X.shape
        sizes = [t.shape[0] for t in tables]
        codes = gin_edge_codes(g, edge_feats, sizes)
        tab, R = concat_tables(tables)
        T = len(tables)
        rows = GEMM_ALGO == "f16x2" and ROW_SCALES
        A = gin_agg(X, D, g, codes, tab, R, T, rows=rows)
        _, w1, h1, lm1 = linear_forward(A, w1, b1, act=1)
        if DEBUG_CAPTURE is not None:  # the ReLU sides the product took (parity tests)
            DEBUG_CAPTURE.setdefault("gin_hidden", []).append(h1.detach().clone())
        _, w2, out, lm2 = linear_forward(h1, w2, b2)
        bctx = None
        if bn is not None:
            if bn.momentum is None:
                raise ValueError("BatchNorm1d: momentum=None (cumulative average) is not implemented on the HIP path")
            training = bn.training or bn.running_mean is None
            bctx = _StageCtx((True, bn_w is not None, bn_b is not None))
            out = BatchNorm1dFunction.forward(bctx, out, bn_w, bn_b, bn.running_mean, bn.running_var,
                                              bn.num_batches_tracked if training else None, training, bn.momentum,
                                              bn.eps)
        ctx.scale = 1.0
        if act:
            call("mvml_relu_f32", out.numel(), ptr(out), ptr(out), _stream(out.device))
            if DEBUG_CAPTURE is not None:
                DEBUG_CAPTURE.setdefault("gin_out", []).append(out.detach().clone())
            ctx.scale = relu_dropout_(out, p)
        ctx.save_for_backward(A, w1, h1, w2, out if act else None)
        ctx.state = (g, codes, R, T, lm1, lm2, bctx, tables)
        return out

    @staticmethod
    def backward(ctx, g_out):
        A, w1, h1, w2, out = ctx.saved_tensors
        g, codes, R, T, lm1, lm2, bctx, tables = ctx.state
        N, D = A.shape
        dev = A.device
        gy = _c(g_out)
        if out is not None:
            g_pre = torch.empty_like(gy)
            call("mvml_relu_bwd", gy.numel(), ptr(out), ptr(gy), ptr(g_pre), float(ctx.scale), _stream(dev))
            gy = g_pre
        g_bnw = g_bnb = None
        if bctx is not None:
            gy, g_bnw, g_bnb = BatchNorm1dFunction.backward(bctx, gy)[:3]
        gh1, gw2, gb2 = linear_backward(h1, w2, gy, lm2)
        g_hid = torch.empty_like(gh1)
        call("mvml_relu_bwd", gh1.numel(), ptr(h1), ptr(gh1), ptr(g_hid), 1.0, _stream(dev))
        gA, gw1, gb1 = linear_backward(A, w1, g_hid, lm1)
        dE = gin_edge_emb_grad(gA, D, g, codes, R, T)
        gX = gcn_agg(gA, D, D, g, (None, None), transpose=True) if ctx.needs_input_grad[0] else None
        return (gX, gw1, gb1, gw2, gb2, g_bnw, g_bnb, None, None, None, None, None, *_split_rows(dE, tables))


_EMBED_STATUS = {}


def embed_status(dev):
    """The int32 device counter of atom categories that lay outside their embedding table (clamped
    into it by mvml_embed_sum_fwd) since the process started; read it with .item() when wanted —
    the forward never synchronises for it."""
    t = _EMBED_STATUS.get(str(dev))
    if t is None:
        t = _EMBED_STATUS[str(dev)] = zeros(1, dtype=torch.int32, device=dev)
    return t


class EmbedSumFunction(torch.autograd.Function):
    """sum_t node_embeddings[t](idx_t) of dgllife's GIN.forward: one pass over the atoms
    (mvml_embed_sum_fwd), the tables' gradient by the two-stage sum of mvml_embed_sum_bwd.
    node_feats: the T integer vectors [N]; tables: the T weights [n_t, D]."""

    @staticmethod
    def forward(ctx, node_feats, *tables):
        for t in tables:
            _check_cuda_f32(t, "node_embeddings")
        dev = tables[0].device
        N = node_feats[0].shape[0]
        idx = _index_tensors(node_feats, N, dev, "categorical_node_feats")
        if len(idx) != len(tables):
            raise ValueError(f"{len(tables)} node tables but {len(idx)} categorical node feature tensors")
        tab, R = concat_tables(tables)
        D = tab.shape[1]
        out = torch.empty((N, D), dtype=torch.float32, device=dev)
        sizes = [t.shape[0] for t in tables]
        _lib.call_tag[0] = {"layer": f"D{D}", "bytes": embed_sum_fwd_bytes(N, len(idx), D, R)}
        call("mvml_embed_sum_fwd", N, *_table_args(idx, sizes), ptr(tab), D, D, ptr(out), D, ptr(embed_status(dev)),
             _stream(dev))
        ctx.state = (idx, sizes, R, D, tables)
        return out

    @staticmethod
    def backward(ctx, g_out):
        idx, sizes, R, D, tables = ctx.state
        G = _rows_f32(g_out)
        N = G.shape[0]
        dev = G.device
        dtab = torch.empty((R, D), dtype=torch.float32, device=dev)
        wp, wn = _emb_grad_ws(N, R, D, dev)
        _lib.call_tag[0] = {"layer": f"D{D}", "bytes": embed_sum_bwd_bytes(N, len(idx), D, R)}
        call("mvml_embed_sum_bwd", N, *_table_args(idx, sizes), ptr(G), G.stride(0), D, ptr(dtab), wp, wn,
             _stream(dev))
        return (None, *_split_rows(dtab, tables))


class SegmentPoolFunction(torch.autograd.Function):
    """dgl's SumPooling / AvgPooling / MaxPooling over the molecules of the device batch g
    (mvml_segment_pool_fwd / _bwd): mode "sum", "mean" or "max"; returns (B, D)."""

    @staticmethod
    def forward(ctx, X, g, mode):
        _check_cuda_f32(X, "feats")
        if mode not in POOL_MODES:
            raise ValueError(f"readout must be one of {sorted(POOL_MODES)}, got {mode!r}")
        X = _rows_f32(X)
        N, D = X.shape
        B = g.batch_size
        dev = X.device
        out = torch.empty((B, D), dtype=torch.float32, device=dev)
        argmax = torch.empty((B, D), dtype=torch.int32, device=dev) if mode == "max" else None
        _lib.call_tag[0] = {"layer": f"D{D}", "bytes": segment_pool_bytes(B, N, D, mode)}
        call("mvml_segment_pool_fwd", B, N, D, POOL_MODES[mode], ptr(g.node_offsets), ptr(X), X.stride(0), ptr(out), D,
             ptr(argmax), D, _stream(dev))
        if DEBUG_CAPTURE is not None and argmax is not None:  # the atoms the product took at ties
            DEBUG_CAPTURE.setdefault("pool_argmax", []).append(argmax.detach().clone())
        ctx.save_for_backward(argmax)
        ctx.state = (g, mode, N, D)
        return out

    @staticmethod
    def backward(ctx, g_out):
        (argmax,) = ctx.saved_tensors
        g, mode, N, D = ctx.state
        G = _rows_f32(g_out)
        B = g.batch_size
        # (rows of atoms outside every molecule cannot exist: node_offsets covers [0, N))
        gX = torch.empty((N, D), dtype=torch.float32, device=G.device)
        _lib.call_tag[0] = {"layer": f"D{D}", "bytes": segment_pool_bytes(B, N, D, mode)}
        call("mvml_segment_pool_bwd", B, N, D, POOL_MODES[mode], ptr(g.node_offsets), ptr(G), G.stride(0), ptr(argmax),
             D, ptr(gX), D, _stream(G.device))
        return gX, None, None


class ForkFunction(torch.autograd.Function):
    """x for two consumers (GIN's jumping knowledge: h_l feeds layer l + 1 and the JK): the two
    gradients that meet at x are added by mvml_add_cols_f32 here, not by the autograd engine."""

    @staticmethod
    def forward(ctx, x):
        return x.view_as(x), x.view_as(x)

    @staticmethod
    def backward(ctx, ga, gb):
        if ga is None or gb is None:  # one consumer took no gradient
            return gb if ga is None else ga
        ga, gb = _rows_f32(ga), _rows_f32(gb)
        s = copy2d(torch.empty(ga.shape, dtype=torch.float32, device=ga.device), ga)
        M, D = s.shape
        if M:
            call("mvml_add_cols_f32", M, D, ptr(gb), gb.stride(0), ptr(s), D, _stream(s.device))
        return s


class JKConcatFunction(torch.autograd.Function):
    """torch.cat([h_0, ..., h_L], dim=1) by mvml_copy_cols into column blocks; the backward copies
    each block out again."""

    @staticmethod
    def forward(ctx, *hs):
        N = hs[0].shape[0]
        ctx.widths = [h.shape[1] for h in hs]
        out = torch.empty((N, sum(ctx.widths)), dtype=torch.float32, device=hs[0].device)
        o = 0
        for h in hs:
            _check_cuda_f32(h, "h")
            if N:
                copy2d(out[:, o:o + h.shape[1]], _rows_f32(h))
            o += h.shape[1]
        return out

    @staticmethod
    def backward(ctx, g):
        g = _rows_f32(g)
        N = g.shape[0]
        out, o = [], 0
        for w in ctx.widths:
            t = torch.empty((N, w), dtype=torch.float32, device=g.device)
            out.append(copy2d(t, g[:, o:o + w]) if N else t)
            o += w
        return tuple(out)


class JKSumFunction(torch.autograd.Function):
    """h_0 + ... + h_L, added in that order by mvml_add_cols_f32 onto a copy of h_0; every input's
    gradient is the output's."""

    @staticmethod
    def forward(ctx, *hs):
        for h in hs:
            _check_cuda_f32(h, "h")
        ctx.n = len(hs)
        h0 = _rows_f32(hs[0])
        out = copy2d(torch.empty(h0.shape, dtype=torch.float32, device=h0.device), h0)
        M, D = out.shape
        for h in hs[1:]:
            h = _rows_f32(h)
            if M:
                call("mvml_add_cols_f32", M, D, ptr(h), h.stride(0), ptr(out), D, _stream(out.device))
        return out

    @staticmethod
    def backward(ctx, g):
        return (g,) * ctx.n
