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


def agg_fwd_bytes(N, E, H, F, out_cols, res_cols, table_rows=None):
    """Algorithmic HBM bytes of one mvml_gat_agg_fwd: read Z and R once,
    rowptr, src ids, el/er; write the layer output and the saved attention.  R is the
    head-mean residual (F columns) in mean mode.  table_rows (mvml_gat_agg_fwd_map): Z and R are
    the rows of a table read once, plus one row index per atom."""
    zr = (H * F + res_cols) * (N if table_rows is None else table_rows) + (0 if table_rows is None else N)
    return 4 * (zr + 2 * N * H + (N + 1) + E + N * out_cols + E * H)


def agg_bwd_bytes(N, E, H, F, gout_cols, mode, table_rows=None):
    """Algorithmic bytes of mvml_gat_agg_bwd: read Z, el/er, g_out (+ out for ELU'), the saved
    attention, both CSRs; write gY = [dZ_agg | dR | d el | d er].  table_rows
    (mvml_gat_agg_bwd_map): Z is the rows of a table read once, plus one row index per atom."""
    rw = F if mode == MODE_MEAN else H * F
    z = N * H * F if table_rows is None else table_rows * H * F + N
    reads = z + 2 * N * H + N * gout_cols + (N * H * F if mode == 0 else 0) + E * H
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


# Layer 1 over the distinct atom-feature rows: a device batch numbers the rows of its resident
# feature buffer (batching.FeatMap, csrc/feat_classes.hip: a few hundred classes among 1.75 M
# atoms); the GAT layer that is handed that buffer projects one row per class and the aggregation
# reads the table through the class ids (mvml_gat_agg_fwd_map / mvml_gat_agg_bwd_map) — bitwise
# the materialised path.  MVML_FEAT_CLASSES=0: no map is built or used.
FEAT_CLASSES = os.environ.get("MVML_FEAT_CLASSES", "1") != "0"


def fold_classes(buf, fm):
    """Record that fm numbers the rows of the feature buffer buf."""
    _remember(buf, "_mvml_classes", fm)


def feat_map_of(g, Xp):
    """The class map of Xp's rows if Xp is batch g's own feature buffer (the batch builds the map
    the first time it is asked: BatchedMolGraph.feat_map_for), unchanged since the map was
    recorded (same rule as known_amax), else None."""
    ask = getattr(g, "feat_map_for", None) if FEAT_CLASSES else None
    fm = ask(Xp) if ask is not None else None
    rec = _recall(Xp, "_mvml_classes") if fm is not None else None
    return fm if rec is not None and rec[0] is fm else None


def map_layout_ok(sep, bias):
    """Whether the row-mapped aggregation entries take this layer: the projection-row layout with
    a bias (they refuse the separate-residual instances: identity / no residual, no bias)."""
    return not sep and bias is not None


def gather_rows(table, ld, cols, idx, rows, offset=0, ldd=None):
    """out[r, :cols] = table[idx[r], offset : offset + cols] (mvml_gather_rows); out [rows, ldd]."""
    out = torch.empty((rows, ldd or cols), dtype=torch.float32, device=table.device)
    call("mvml_gather_rows", rows, cols, ctypes.c_void_p(table.data_ptr() + 4 * offset), ld, ptr(idx),
         ptr(out), ldd or cols, _stream(table.device))
    return out


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
        # the batch's own feature buffer with a class map: one projection row per class
        fm = feat_map_of(g, Xp) if ((algo or GEMM_ALGO) == "f16x2" and ROW_SCALES
                                    and map_layout_ok(sep, bias)) else None
        if (algo or GEMM_ALGO) == "f16x2":
            amx = zeros(4, dtype=torch.int32, device=dev)  # [X, Wcat, gY (bwd), out]
            if ROW_SCALES:
                # the projection splits every atom row with its own scale; max |X| (the weight
                # gradient's A-side scale) is the max of the row maxima (N floats, not N x Fp).
                # Layer 1's rows are those of the resident atom features (the pad columns are
                # zeros): computed once and recorded on the feature tensor itself.  (Xp's pad
                # columns are zeros: the whole padded row, float4 loads, has the same |max| as
                # its Fin features)
                if fm is not None:
                    # the class rows' scales; their max is max |X| (the same set of rows)
                    xr = absmax_rows(fm.Xc, fm.C, Fp, Fp)
                    absmax(xr, fm.C, 1, 1, amx, 0)
                else:
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
            Y = torch.empty((N if fm is None else fm.C, ldy), dtype=torch.float32, device=dev)
            if fm is not None:
                # Y[c] = the projection of class c's row: a row of the product depends on that row,
                # the weights and its scale only, so Y[cls[a]] is bitwise atom a's projection
                gemm(fm.Xc, Wcat, fm.C, C + 2 * H, Fp, 0, 0, Fp, Fp, Y, ldy, amax=(None, slot(amx, 1)),
                     arows=xr, bil4=wil, role="gat_proj")
            elif xr is not None:
                gemm(Xp, Wcat, N, C + 2 * H, Fp, 0, 0, Fp, Fp, Y, ldy, amax=(None, slot(amx, 1)),
                     arows=xr, bil4=wil, role="gat_proj")
            elif amx is not None:
                gemm(Xp, Wcat, N, C + 2 * H, Fp, 0, 0, Fp, Fp, Y, ldy, amax=(slot(*ax), slot(amx, 1)))
            else:
                gemm(Xp, Wcat, N, C + 2 * H, Fp, 0, 0, Fp, Fp, Y, ldy, algo="bf16")
            # (a native slice copy: torch's strided copy splits into 32-bit-indexable pieces,
            # 8 launches for a 1.75 M-atom batch)
            if fm is not None:
                elr = gather_rows(Y, ldy, 2 * H, fm.cls, N, offset=C)
            else:
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
        with _fwd_path(g, mode):
            while True:
                # yrow: the aggregation reads atom a's projection row at Y[yrow[a]] (the *_map
                # entries, filed under the plain entry's timings); a path that has no row-mapped
                # instances refuses before it launches anything, and Y is materialised instead
                yrow = None if fm is None else fm.cls
                sfx, extra = ("", ()) if yrow is None else ("_map", (ptr(yrow),))
                _lib.call_tag[0] = {"layer": f"H{H}xF{F}",
                                    "bytes": agg_fwd_bytes(N, E, H, F, out_cols, 0 if res_kind == RES_NONE else rw,
                                                           None if fm is None else fm.C)}
                try:
                    if not sep and bias is not None:
                        call("mvml_gat_agg_fwd" + sfx, N, ptr(g.node_groups), g.num_node_groups, ptr(g.in_rowptr),
                             ptr(g.in_src), ptr(Y), ldy, H, F, ptr(elr), ptr(_c(bias)), float(slope), int(mode),
                             ptr(out), ptr(attn), slot(amx, 3), ptr(orows), st, *extra, timed_as="mvml_gat_agg_fwd")
                    else:
                        rp = ctypes.c_void_p(Y.data_ptr() + 4 * HF) if not sep else ptr(R)
                        call("mvml_gat_agg_fwd_res" + sfx, N, ptr(g.node_groups), g.num_node_groups,
                             ptr(g.in_rowptr), ptr(g.in_src), ptr(Y), ldy, H, F, ptr(elr), rp, ldr if sep else ldy,
                             ptr(_c(bias)) if bias is not None else None, float(slope), int(mode),
                             ptr(out), ptr(attn), slot(amx, 3), ptr(orows), st, *extra,
                             timed_as="mvml_gat_agg_fwd_res")
                    break
                except _lib.MvmlError as e:
                    if fm is None or "the row map needs" not in str(e):  # the entry's own refusal only
                        raise
                    Y, fm = gather_rows(Y, ldy, ldy, fm.cls, N), None
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
            DEBUG_CAPTURE.setdefault("mapped_fwd", []).append((fm is not None, Y.shape[0]))
        ctx.save_for_backward(Xp, Wcat, Y, attn, elr, out, attn_l, attn_r, attn_lr)
        ctx.Fin = Fin
        ctx.g, ctx.H, ctx.F, ctx.slope, ctx.mode, ctx.ldy = g, H, F, slope, mode, ldy
        ctx.algo = algo
        ctx.res_kind, ctx.has_bias = res_kind, bias is not None
        ctx.amx = amx
        ctx.ax = ax
        ctx.wil = wil
        ctx.yrow = None if fm is None else fm.cls  # Y is the class table: rows through yrow
        return out

    @staticmethod
    def backward(ctx, g_out):
        Xp, Wcat, Y, attn, elr, out, attn_l, attn_r, attn_lr = ctx.saved_tensors
        g, H, F, mode, ldy = ctx.g, ctx.H, ctx.F, ctx.mode, ctx.ldy
        yrow = ctx.yrow
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
            while True:  # (yrow: as in the forward)
                sfx, extra = ("", ()) if yrow is None else ("_map", (ptr(yrow),))
                _lib.call_tag[0] = {"layer": f"H{H}xF{F}",
                                    "bytes": agg_bwd_bytes(N, g.num_edges(), H, F, g_out.shape[1], mode,
                                                           None if yrow is None else Y.shape[0])}
                try:
                    if sep:
                        call("mvml_gat_agg_bwd_res" + sfx, N, ptr(g.node_groups), g.num_node_groups,
                             ptr(g.in_rowptr), ptr(g.in_src), ptr(g.out_rowptr), ptr(g.out_dst), ptr(g.out_inslot),
                             ptr(Y), ldy, ptr(elr), ptr(attn), ptr(out), ptr(g_out), H, F, float(ctx.slope),
                             int(mode), ptr(gY), ldg, C, ptr(gR), ldgr, slot(ctx.amx, 2), ptr(gyr), wp, wn, st,
                             *extra, timed_as="mvml_gat_agg_bwd_res")
                    else:
                        call("mvml_gat_agg_bwd" + sfx, N, ptr(g.node_groups), g.num_node_groups, ptr(g.in_rowptr),
                             ptr(g.in_src), ptr(g.out_rowptr), ptr(g.out_dst), ptr(g.out_inslot), ptr(Y), ldy,
                             ptr(elr), ptr(attn), ptr(out), ptr(g_out), H, F, float(ctx.slope), int(mode), ptr(gY),
                             ldg, slot(ctx.amx, 2), ptr(gyr), wp, wn, st, *extra, timed_as="mvml_gat_agg_bwd")
                    break
                except _lib.MvmlError as e:
                    if yrow is None or "the row map needs" not in str(e):
                        raise
                    Y, yrow = gather_rows(Y, ldy, ldy, yrow, N), None
        amx = ctx.amx  # slot 2 = max |gY|, folded in by mvml_gat_agg_bwd's stores
        if DEBUG_CAPTURE is not None:
            DEBUG_CAPTURE.setdefault("mapped_bwd", []).append(yrow is not None)
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


# ---- AttentiveFP (csrc/afp_agg.hip, csrc/gru.hip, csrc/attn_pool.hip; DESIGN.md "AttentiveFP") ----
AFP_SLOPE = 0.01         # torch's LeakyReLU default, AttentiveFP's everywhere
AFP_MAX_EDGE_FEATS = 32  # bond features per edge (mvml_afp_context_fwd)
AFP_MAX_WIDTH = 1024     # graph_feat_size


def afp_context_fwd_bytes(N, E, G, De):
    """Algorithmic HBM bytes of one mvml_afp_context_fwd: P read and s written once, the row
    pointers, the neighbour ids, the padded bond rows, t, the attention (re-gathers not counted)."""
    return 4 * (2 * N * G + N + 1 + E + E * _round4(De) + N + E + (De + 2) * G)


def afp_context_bwd_bytes(N, E, G, De):
    """Algorithmic bytes of one mvml_afp_context_bwd: stage 1 reads P, s, g_s, the bond rows and
    the attention, parks two scalars per slot, re-reads them and writes d_pre and g_t; stage 2 reads P, g_s, the bond rows, the attention and
    d_pre and writes gP; both write and re-read their partial rows."""
    Pn = _lib.lib().mvml_afp_partial_rows(N)
    idx = 2 * (N + 1) + 3 * E
    return 4 * (5 * N * G + N * G + 2 * E * _round4(De) + 8 * E + 2 * N + idx + 2 * Pn * (De + 2) * G)


def gru_cell_bytes(M, D, backward):
    """Algorithmic bytes of mvml_gru_cell_fwd (gi, gh, h in; out, save out) or _bwd."""
    return 4 * M * D * ((3 + 3 + 1 + 1 + 4) if not backward else (4 + 1 + 1 + 1 + 3 + 3 + 1))


def attn_pool_bytes(B, N, D, backward):
    """Algorithmic bytes of mvml_attn_pool_fwd (X once, r, attn) or _bwd (X once, gX, r, g_r, attn)."""
    return 4 * ((N * D + B * D + N + B) if not backward else (2 * N * D + 2 * B * D + N + 2 * B))


def _off(t, floats):
    """The device pointer `floats` elements past t's first."""
    return ctypes.c_void_p(t.data_ptr() + 4 * floats)


def _dense(view):
    """A contiguous copy of a 2-D (or 1-D) float32 view with unit column stride (mvml_copy_cols)."""
    return copy2d(torch.empty(view.shape, dtype=torch.float32, device=view.device), view)


def afp_edge_rows(g, edge_feats):
    """The [E, round_up(De, 4)] bond rows of the device batch g in in-CSR slot order, zero-padded
    (mvml_afp_edge_rows).  Made once per (batch, feature tensor) and kept on the batch as GIN's
    codes are; BatchedMolGraph.recollate() drops it."""
    _check_cuda_f32(edge_feats, "edge_feats")
    E = g.num_edges()
    if edge_feats.dim() != 2 or edge_feats.shape[0] != E or not 1 <= edge_feats.shape[1] <= AFP_MAX_EDGE_FEATS:
        raise ValueError(f"edge_feats: a float [E = {E}, 1..{AFP_MAX_EDGE_FEATS}] tensor in edge-id order expected, "
                         f"got {tuple(edge_feats.shape)}")
    key = (edge_feats.data_ptr(), edge_feats._version, tuple(edge_feats.shape), tuple(edge_feats.stride()))
    cache = g._dev.setdefault("afp_rows", {})
    if key not in cache:
        e = _c(edge_feats)
        De = e.shape[1]
        rows = torch.empty((max(E, 1), _round4(De)), dtype=torch.float32, device=g.device)
        call("mvml_afp_edge_rows", E, De, ptr(g.in_eid), ptr(e), De, ptr(rows), _stream(g.device))
        cache[key] = (rows, edge_feats)  # (the given tensor is kept: its address is the key)
    return cache[key][0]


def _gru_forward(x, h, w_ih, w_hh, b_ih, b_hh, relu):
    """relu?(GRUCell(x, h)): the two gate products on the GEMM, the gates in mvml_gru_cell_fwd.
    Returns (out, state); state is what _gru_backward takes beside `out` (kept apart: where out is
    an autograd node's output it goes through save_for_backward, not into the node's own state)."""
    x, w_ih, gi, lmi = linear_forward(x, w_ih, None)
    h, w_hh, gh, lmh = linear_forward(h, w_hh, None)
    M, D = h.shape
    dev = h.device
    out = torch.empty((M, D), dtype=torch.float32, device=dev)
    save = torch.empty((M, 4 * D), dtype=torch.float32, device=dev)
    _lib.call_tag[0] = {"layer": f"D{D}", "bytes": gru_cell_bytes(M, D, False)}
    call("mvml_gru_cell_fwd", M, D, ptr(gi), ptr(gh), ptr(_c(b_ih)), ptr(_c(b_hh)), ptr(h), D, int(relu), ptr(out), D,
         ptr(save), _stream(dev))
    return out, (x, h, w_ih, w_hh, lmi, lmh, save, int(relu))


def _gru_backward(state, out, g_out, need_gx=True):
    """(g_x, g_h, g_w_ih, g_w_hh, g_b_ih, g_b_hh) of _gru_forward; g_h holds the direct z g term
    plus the hidden product's share (accumulated by that product, beta = 1).  out: the forward's
    output, read for the ReLU's sides only (None without a ReLU)."""
    x, h, w_ih, w_hh, lmi, lmh, save, relu = state
    M, D = h.shape
    dev = h.device
    g_out = _rows_f32(g_out)
    g_gi = torch.empty((M, 3 * D), dtype=torch.float32, device=dev)
    g_gh = torch.empty((M, 3 * D), dtype=torch.float32, device=dev)
    g_h = torch.empty((M, D), dtype=torch.float32, device=dev)
    _lib.call_tag[0] = {"layer": f"D{D}", "bytes": gru_cell_bytes(M, D, True)}
    call("mvml_gru_cell_bwd", M, D, ptr(save), ptr(h), D, ptr(out), D, ptr(g_out), g_out.stride(0), relu, ptr(g_gi),
         ptr(g_gh), ptr(g_h), D, _stream(dev))
    g_x, g_wih, g_bih = linear_backward(x, w_ih, g_gi, lmi, need_gx=need_gx)
    g_h, g_whh, g_bhh = linear_backward(h, w_hh, g_gh, lmh, gx_acc=g_h)
    return g_x, g_h, g_wih, g_whh, g_bih, g_bhh


def _elu_(x, g=None, bias=None):
    """x = elu(x + bias) in place; g: the batch whose atoms without in-edges take no bias."""
    M, D = x.shape
    call("mvml_afp_bias_elu", M, D, ptr(g.in_rowptr) if g is not None else None, ptr(x), D,
         None if bias is None else ptr(_c(bias)), _stream(x.device))
    return x


def _elu_backward(out, g_out, g=None):
    """The gradient before _elu_ (zero rows for the atoms it masked)."""
    M, D = out.shape
    g_out = _rows_f32(g_out)
    gx = torch.empty((M, D), dtype=torch.float32, device=out.device)
    call("mvml_afp_bias_elu_bwd", M, D, ptr(g.in_rowptr) if g is not None else None, ptr(out), D, ptr(g_out),
         g_out.stride(0), ptr(gx), D, _stream(out.device))
    return gx


class AFPContextFunction(torch.autograd.Function):
    """dgllife 0.3.0 GetContext.forward (restated; parity with dgllife is unpinned) as ONE autograd
    node.  One GEMM over the atom features gives [x Wn^T + bn | P = x W1n^T]; hv_new = leaky of the
    first half; t = w2n . hv_new + b2 per atom; mvml_afp_context_fwd runs the bond-aware edge
    softmax and its weighted sum s without any [E, G] tensor; c = elu(We s + be [deg > 0]) is a
    node-level GEMM and mvml_afp_bias_elu; h = relu(GRUCell(c, hv_new)).  The Fn + De and 2G wide
    weights are split by columns here, per call.  Bond features get no gradient."""

    @staticmethod
    def forward(ctx, X, edge_feats, g, Wn, bn, W1, b1, W2, b2, We, be, w_ih, w_hh, b_ih, b_hh):
        _check_cuda_f32(X, "node_feats")
        for p in (Wn, bn, W1, b1, W2, b2, We, be, w_ih, w_hh, b_ih, b_hh):
            _check_cuda_f32(p, "GetContext parameters")
        X, Xp = _padded_input(X)
        N, Fn = X.shape
        Fp = Xp.shape[1]
        G = Wn.shape[0]
        De = W1.shape[1] - Fn
        dev = X.device
        st = _stream(dev)
        E = g.num_edges()
        rows = afp_edge_rows(g, edge_feats)
        if edge_feats.shape[1] != De:
            raise ValueError(f"GetContext: {De} bond features expected, got {edge_feats.shape[1]}")
        Wcat = zeros((2 * G, Fp), device=dev)
        copy2d(Wcat[:G, :Fn], Wn)
        copy2d(Wcat[G:, :Fn], W1[:, :Fn])
        bcat = zeros(2 * G, device=dev)
        copy2d(bcat[:G], bn)
        _, _, Y, lmY = linear_forward(Xp, Wcat, bcat)
        hv = torch.empty((N, G), dtype=torch.float32, device=dev)
        call("mvml_leaky_f32", N, G, ptr(Y), 2 * G, ptr(hv), G, AFP_SLOPE, st)
        W2 = _c(W2)
        w2n = W2[:, :G]
        _, w2n, t, lmt = linear_forward(hv, w2n, b2)
        W1eT = torch.empty((De, G), dtype=torch.float32, device=dev)
        W1 = _c(W1)
        call("mvml_transpose", G, De, _off(W1, Fn), Fn + De, ptr(W1eT), G, st)
        b1 = _c(b1)
        s = torch.empty((N, G), dtype=torch.float32, device=dev)
        attn = torch.empty(max(E, 1), dtype=torch.float32, device=dev)
        _lib.call_tag[0] = {"layer": f"G{G}xDe{De}", "bytes": afp_context_fwd_bytes(N, E, G, De)}
        call("mvml_afp_context_fwd", N, ptr(g.in_rowptr), ptr(g.in_src), _off(Y, G), 2 * G, G, ptr(rows), De, ptr(W1eT),
             ptr(b1), _off(W2, G), ptr(t), ptr(s), G, ptr(attn), st)
        _, We, c, lmc = linear_forward(s, We, None)
        _elu_(c, g, be)
        h, gst = _gru_forward(c, hv, w_ih, w_hh, b_ih, b_hh, True)
        ctx.state = (g, rows, Xp, Wcat, lmY, Y, hv, w2n, lmt, t, W1eT, b1, W2, s, attn, We, lmc, c, gst, Fn, De)
        ctx.save_for_backward(h)
        return h

    @staticmethod
    def backward(ctx, g_out):
        g, rows, Xp, Wcat, lmY, Y, hv, w2n, lmt, t, W1eT, b1, W2, s, attn, We, lmc, c, gst, Fn, De = ctx.state
        N, G = hv.shape
        E = g.num_edges()
        dev = hv.device
        st = _stream(dev)
        g_c, g_hv, g_wih, g_whh, g_bih, g_bhh = _gru_backward(gst, ctx.saved_tensors[0], g_out)
        g_cpre = _elu_backward(c, g_c, g)
        g_s, g_We, _ = linear_backward(s, We, g_cpre, lmc, need_gb=False)
        g_be = torch.empty(G, dtype=torch.float32, device=dev)
        colsum(g_cpre, N, G, G, g_be)  # (the masked atoms' rows are zero)
        gY = torch.empty((N, 2 * G), dtype=torch.float32, device=dev)
        g_t = torch.empty((N, 1), dtype=torch.float32, device=dev)
        g_W2 = torch.empty((1, 2 * G), dtype=torch.float32, device=dev)
        g_w1b = torch.empty((De + 1, G), dtype=torch.float32, device=dev)
        wp, wn = _lib.ws_ptr_size(_lib.lib().mvml_afp_context_bwd_workspace_size(N, E, G, De), dev)
        _lib.call_tag[0] = {"layer": f"G{G}xDe{De}", "bytes": afp_context_bwd_bytes(N, E, G, De)}
        call("mvml_afp_context_bwd", N, E, ptr(g.in_rowptr), ptr(g.in_src), ptr(g.out_rowptr), ptr(g.out_dst),
             ptr(g.out_inslot), _off(Y, G), 2 * G, G, ptr(rows), De, ptr(W1eT), ptr(b1), _off(W2, G), ptr(t), ptr(s), G,
             ptr(attn), ptr(g_s), G, _off(gY, G), 2 * G, ptr(g_t), _off(g_W2, G), ptr(g_w1b), wp, wn, st)
        g_hv, g_w2n, g_b2 = linear_backward(hv, w2n, g_t, lmt, gx_acc=g_hv)
        copy2d(g_W2[:, :G], g_w2n)
        call("mvml_leaky_bwd_f32", N, G, ptr(hv), G, ptr(g_hv), G, ptr(gY), 2 * G, AFP_SLOPE, st)
        gXp, gWcat, gbcat = linear_backward(Xp, Wcat, gY, lmY, need_gx=ctx.needs_input_grad[0])
        g_W1 = torch.empty((G, Fn + De), dtype=torch.float32, device=dev)
        copy2d(g_W1[:, :Fn], gWcat[G:, :Fn])
        call("mvml_transpose", De, G, ptr(g_w1b), G, _off(g_W1, Fn), Fn + De, st)
        gX = _dense(gXp[:, :Fn]) if gXp is not None else None
        return (gX, None, None, _dense(gWcat[:G, :Fn]), _dense(gbcat[:G]), g_W1, _dense(g_w1b[De]), g_W2, g_b2, g_We,
                g_be, g_wih, g_whh, g_bih, g_bhh)


class AFPGNNLayerFunction(torch.autograd.Function):
    """dgllife 0.3.0 GNNLayer.forward (restated) as ONE autograd node: logits leaky(w_d . h_v +
    w_s . h_u + b) are a one-head GAT's el / er pair, so one GEMM gives [Z = h Wp^T + bp | el | er]
    and the existing mvml_gat_agg_fwd_res (H = 1, flatten + ELU, no residual, no bias, slope 0.01)
    gives elu(sum_e a_e Z[u]); then h' = relu(GRUCell(that, h)) and BatchNorm1d (bn: the parameter
    container) on the project's kernel."""

    @staticmethod
    def forward(ctx, h, g, w_edge, b_edge, Wp, bp, w_ih, w_hh, b_ih, b_hh, bn_w, bn_b, bn):
        _check_cuda_f32(h, "node_feats")
        h = _c(h)
        N, G = h.shape
        dev = h.device
        st = _stream(dev)
        E = g.num_edges()
        C = G + 4  # [Z | el | er | 2 pad]
        Wz = zeros((C, G), device=dev)
        copy2d(Wz[:G], _c(Wp))
        w_edge = _c(w_edge)
        copy2d(Wz[G:G + 1], w_edge[:, G:])      # el: the source term
        copy2d(Wz[G + 1:G + 2], w_edge[:, :G])  # er: the destination term (+ the bias)
        bz = zeros(C, device=dev)
        copy2d(bz[:G], bp)
        copy2d(bz[G + 1:G + 2], b_edge)
        _, _, Y, lmY = linear_forward(h, Wz, bz)
        elr = torch.empty((N, 2), dtype=torch.float32, device=dev)
        call("mvml_copy_cols", N, 2, _off(Y, G), C, ptr(elr), 2, st)
        c = torch.empty((N, G), dtype=torch.float32, device=dev)
        attn = torch.empty((max(E, 1), 1), dtype=torch.float32, device=dev)
        _lib.call_tag[0] = {"layer": f"H1xF{G}", "bytes": agg_fwd_bytes(N, E, 1, G, G, 0)}
        call("mvml_gat_agg_fwd_res", N, ptr(g.node_groups), g.num_node_groups, ptr(g.in_rowptr), ptr(g.in_src), ptr(Y),
             C, 1, G, ptr(elr), None, 0, None, AFP_SLOPE, MODE_FLATTEN_ELU, ptr(c), ptr(attn), None, None, st)
        out, gst = _gru_forward(c, h, w_ih, w_hh, b_ih, b_hh, True)
        bctx = _StageCtx((True, True, True))
        training = bn.training or bn.running_mean is None
        if bn.momentum is None:
            raise ValueError("BatchNorm1d: momentum=None (cumulative average) is not implemented on the HIP path")
        y = BatchNorm1dFunction.forward(bctx, out, bn_w, bn_b, bn.running_mean, bn.running_var,
                                        bn.num_batches_tracked if training else None, training, bn.momentum, bn.eps)
        ctx.state = (g, h, Wz, lmY, Y, elr, c, attn, gst, out, bctx)
        return y

    @staticmethod
    def backward(ctx, g_y):
        g, h, Wz, lmY, Y, elr, c, attn, gst, out, bctx = ctx.state
        N, G = h.shape
        C = G + 4
        dev = h.device
        st = _stream(dev)
        g_out, g_bnw, g_bnb = BatchNorm1dFunction.backward(bctx, _c(g_y))[:3]
        g_c, g_h, g_wih, g_whh, g_bih, g_bhh = _gru_backward(gst, out, g_out)
        gY = zeros((N, C), device=dev)  # (the two pad columns stay 0)
        # (a batch without bonds still passes a workspace: the entry wants a pointer)
        wp, wn = _lib.ws_ptr_size(_lib.lib().mvml_gat_agg_bwd_workspace_size(max(g.num_edges(), 1), 1), dev)
        _lib.call_tag[0] = {"layer": f"H1xF{G}", "bytes": agg_bwd_bytes(N, g.num_edges(), 1, G, G, 0)}
        call("mvml_gat_agg_bwd_res", N, ptr(g.node_groups), g.num_node_groups, ptr(g.in_rowptr), ptr(g.in_src),
             ptr(g.out_rowptr), ptr(g.out_dst), ptr(g.out_inslot), ptr(Y), C, ptr(elr), ptr(attn), ptr(c), ptr(g_c), 1, G,
             AFP_SLOPE, MODE_FLATTEN_ELU, ptr(gY), C, G, None, 0, None, None, wp, wn, st)
        g_h, gWz, gbz = linear_backward(h, Wz, gY, lmY, gx_acc=g_h)
        g_wedge = torch.empty((1, 2 * G), dtype=torch.float32, device=dev)
        copy2d(g_wedge[:, G:], gWz[G:G + 1])
        copy2d(g_wedge[:, :G], gWz[G + 1:G + 2])
        return (g_h, None, g_wedge, _dense(gbz[G + 1:G + 2]), _dense(gWz[:G]), _dense(gbz[:G]), g_wih, g_whh, g_bih,
                g_bhh, g_bnw, g_bnb, None)


class AFPReadoutFunction(torch.autograd.Function):
    """dgllife 0.3.0 AttentiveFPReadout.forward (restated) as ONE autograd node: gf = the per-graph
    sum of the atom rows (mvml_segment_pool_fwd), then per timestep u = wg . relu(gf) + bz (a GEMM),
    the softmax-weighted sum r of the atom rows (mvml_attn_pool_fwd), elu(Wp r + bp) at GRAPH level
    (every graph has an atom and the weights sum to 1) and gf = GRUCell(that, gf).  params: per
    timestep (compute_logits weight [1, 2D] and bias, project_nodes weight and bias, the GRUCell's
    four).  All timesteps' atom gradients and the initial sum's add into one gX."""

    @staticmethod
    def forward(ctx, X, g, T, *params):
        _check_cuda_f32(X, "node_feats")
        X = _rows_f32(X)
        N, D = X.shape
        B = g.batch_size
        dev = X.device
        st = _stream(dev)
        gf = torch.empty((B, D), dtype=torch.float32, device=dev)
        call("mvml_segment_pool_fwd", B, N, D, POOL_MODES["sum"], ptr(g.node_offsets), ptr(X), X.stride(0), ptr(gf), D,
             None, D, st)
        steps = []
        for k in range(T):
            wl, bl, Wp, bp, w_ih, w_hh, b_ih, b_hh = params[8 * k:8 * k + 8]
            wl = _c(wl)
            rg = torch.empty_like(gf)
            call("mvml_relu_f32", gf.numel(), ptr(gf), ptr(rg), st)
            _, wg, u, lmu = linear_forward(rg, wl[:, :D], bl)
            r = torch.empty((B, D), dtype=torch.float32, device=dev)
            attn = torch.empty(max(N, 1), dtype=torch.float32, device=dev)
            _lib.call_tag[0] = {"layer": f"D{D}", "bytes": attn_pool_bytes(B, N, D, False)}
            call("mvml_attn_pool_fwd", B, N, D, ptr(g.node_offsets), ptr(X), X.stride(0), _off(wl, D), ptr(u), AFP_SLOPE,
                 ptr(r), D, ptr(attn), st)
            _, Wp, c, lmc = linear_forward(r, Wp, bp)
            _elu_(c)
            gf, gst = _gru_forward(c, gf, w_ih, w_hh, b_ih, b_hh, False)
            steps.append((wl, rg, wg, u, lmu, r, attn, Wp, c, lmc, gst))
        ctx.state = (g, X, steps)
        return gf

    @staticmethod
    def backward(ctx, g_gf):
        g, X, steps = ctx.state
        N, D = X.shape
        B = g.batch_size
        dev = X.device
        st = _stream(dev)
        gX = torch.empty((N, D), dtype=torch.float32, device=dev)
        wp, wn = _lib.ws_ptr_size(_lib.lib().mvml_attn_pool_bwd_workspace_size(B, N, D), dev)
        grads = []
        for k in reversed(range(len(steps))):
            wl, rg, wg, u, lmu, r, attn, Wp, c, lmc, gst = steps[k]
            g_c, g_gf, g_wih, g_whh, g_bih, g_bhh = _gru_backward(gst, None, g_gf)
            g_cpre = _elu_backward(c, g_c)
            g_r, g_Wp, g_bp = linear_backward(r, Wp, g_cpre, lmc)
            g_u = torch.empty((B, 1), dtype=torch.float32, device=dev)
            g_wl = torch.empty((1, 2 * D), dtype=torch.float32, device=dev)
            _lib.call_tag[0] = {"layer": f"D{D}", "bytes": attn_pool_bytes(B, N, D, True)}
            call("mvml_attn_pool_bwd", B, N, D, ptr(g.node_offsets), ptr(X), X.stride(0), _off(wl, D), ptr(u), AFP_SLOPE,
                 ptr(r), D, ptr(attn), ptr(g_r), D, int(k != len(steps) - 1), ptr(gX), D, ptr(g_u), _off(g_wl, D), wp, wn,
                 st)
            g_rg, g_wg, g_bl = linear_backward(rg, wg, g_u, lmu)
            copy2d(g_wl[:, :D], g_wg)
            g_relu = torch.empty_like(g_rg)
            call("mvml_relu_bwd", g_rg.numel(), ptr(rg), ptr(g_rg), ptr(g_relu), 1.0, st)
            call("mvml_add_cols_f32", B, D, ptr(g_relu), D, ptr(g_gf), D, st)
            grads[:0] = [g_wl, g_bl, g_Wp, g_bp, g_wih, g_whh, g_bih, g_bhh]
        g_sum = torch.empty((N, D), dtype=torch.float32, device=dev)
        call("mvml_segment_pool_bwd", B, N, D, POOL_MODES["sum"], ptr(g.node_offsets), ptr(g_gf), D, None, D, ptr(g_sum), D,
             st)
        if steps:
            call("mvml_add_cols_f32", N, D, ptr(g_sum), D, ptr(gX), D, st)
        else:
            gX = g_sum
        return (gX, None, None, *grads)


# ---- MPNN: NNConv on csrc/nnconv.hip ("MPNN") ------------------------------------------
NNCONV_MAX_D = 128  # node_out_feats (mvml_nnconv_fwd)
NNCONV_MAX_H = 256  # edge_hidden_feats


def nnconv_check(who, D, H):
    """The widths mvml_nnconv_* take: multiples of 16, D in [16, 128], H in [16, 256]."""
    for what, v, hi in (("node_out_feats", D, NNCONV_MAX_D), ("edge_hidden_feats", H, NNCONV_MAX_H)):
        if not isinstance(v, int) or v < 16 or v % 16 or v > hi:
            raise ValueError(f"{who}: {what} must be a multiple of 16 in [16, {hi}] on the HIP path (got {v})")


NNCONV_WEIGHT_GRADS = ("fp32", "split_fp16")  # mvml_nnconv_bwd_weight, mvml_nnconv_bwd_weight_f16x2


def nnconv_weight_grad(value):
    if value not in NNCONV_WEIGHT_GRADS:
        raise ValueError(f"NNConv: weight_grad must be one of {NNCONV_WEIGHT_GRADS} (got {value!r})")
    return value


def nnconv_z_image(z, E):
    """max |z| and z split and transposed into MFMA fragment order (mvml_nnconv_split_z): 4 H bytes per
    edge, the operand of mvml_nnconv_bwd_weight_f16x2."""
    H = z.shape[1]
    img = torch.empty(_lib.lib().mvml_nnconv_z_image_bytes(E, H), dtype=torch.uint8, device=z.device)
    call("mvml_nnconv_split_z", E, H, ptr(z), z.stride(0), ptr(img), _stream(z.device))
    return img


def nnconv_flops(E, D, H):
    """2 H D^2 per edge: the flops of one of the three NNConv products (the MFMA work of the
    split-fp16 kernels is three times that, before their K padding)."""
    return 2 * E * H * D * D


def nnconv_slot_dst(g):
    """int32 [E]: the destination atom of every in-CSR slot (mvml_nnconv_slot_dst), made once per
    batch and kept on it; BatchedMolGraph.recollate() drops it."""
    d = g._dev
    if "nnconv_slot_dst" not in d:
        t = torch.empty(max(g.num_edges(), 1), dtype=torch.int32, device=g.device)
        call("mvml_nnconv_slot_dst", g.num_nodes(), ptr(g.in_rowptr), ptr(t), _stream(g.device))
        d["nnconv_slot_dst"] = t
    return d["nnconv_slot_dst"]


def nnconv_image(W2, D, H):
    """max |W2| and W2's two split-fp16 images in MFMA fragment order (mvml_nnconv_split_w2)."""
    nbytes = _lib.lib().mvml_nnconv_image_bytes(D, H)
    if nbytes == 0 or tuple(W2.shape) != (D * D, H):
        raise ValueError(f"NNConv: edge_func must end in a Linear({H}, {D * D}) with widths that are multiples of 16, "
                         f"D <= {NNCONV_MAX_D}, H <= {NNCONV_MAX_H} (weight {tuple(W2.shape)})")
    img = torch.empty(nbytes, dtype=torch.uint8, device=W2.device)
    call("mvml_nnconv_split_w2", D, H, ptr(W2), ptr(img), _stream(W2.device))
    return img


class NNConvShared:
    """What the message-passing steps of one MPNNGNN forward share: W2's image (split once) and, in
    the backward, ONE dz, dW2, db2 and dbias that every step's kernels add onto (their accumulate
    flag), handed to autograd by the step whose backward runs last.  weight_grad "split_fp16" runs
    dW2 on mvml_nnconv_bwd_weight_f16x2: z's image (mvml_nnconv_split_z) is made by the first backward,
    reused by every step's and dropped with the last."""

    def __init__(self, image, steps, weight_grad="fp32"):
        self.image, self.steps, self.done = image, steps, 0
        self.weight_grad, self.z_image = nnconv_weight_grad(weight_grad), None

    def alloc(self, E, D, H, dev):
        f32 = dict(dtype=torch.float32, device=dev)
        self.dz = torch.empty((max(E, 1), H), **f32)
        self.dW2 = torch.empty((D * D, H), **f32)
        self.db2 = torch.empty(D * D, **f32)
        self.dbias = torch.empty(D, **f32)


def nnconv_forward(g, h, z, b2, bias, image, act):
    """(out, S): out = act(NNConv(h)) [N, D] dense, S = the per-destination sums of the source rows
    (the b2 part's operand).  h [N, D] and z [E, H] row-pitched, b2 [D * D] and bias [D] dense."""
    N, D = h.shape
    E, H = g.num_edges(), z.shape[1]
    dev = h.device
    out = torch.empty((N, D), dtype=torch.float32, device=dev)
    wp, wn = _lib.ws_ptr_size(_lib.lib().mvml_nnconv_fwd_workspace_size(E, D), dev)
    _lib.call_tag[0] = {"layer": f"D{D}xH{H}", "flops": nnconv_flops(E, D, H)}
    call("mvml_nnconv_fwd", N, E, ptr(g.in_rowptr), ptr(g.in_src), ptr(h), h.stride(0), D, ptr(z), z.stride(0), H,
         ptr(image), ptr(bias), ptr(out), D, wp, wn, _stream(dev))
    # (mvml_gcn_agg wants its neighbour list: a batch without any bond has none, and S = 0)
    S = gcn_agg(h, h.stride(0), D, g, (None, None)) if E else zeros((N, D), device=dev)
    gemm(S, b2, N, D, D, 0, 1, D, D, out, D, beta=1.0, act=int(act))  # out = act(out + S view(b2))
    return out, S


def nnconv_backward(g, h, z, b2, image, S, out, g_out, act, acc, accumulate):
    """dL/dh [N, D] of nnconv_forward from g_out = dL/d out; dz, dW2, db2 and dbias go into (or,
    accumulate, onto) acc's buffers."""
    N, D = h.shape
    E, H = g.num_edges(), z.shape[1]
    dev = h.device
    st = _stream(dev)
    g_out = _c(g_out)
    if act:
        g_pre = torch.empty_like(out)
        call("mvml_relu_bwd", out.numel(), ptr(out), ptr(g_out), ptr(g_pre), 1.0, st)
    else:
        g_pre = g_out
    L = _lib.lib()
    sd = nnconv_slot_dst(g)
    dH = torch.empty((N, D), dtype=torch.float32, device=dev)
    wp, wn = _lib.ws_ptr_size(L.mvml_nnconv_bwd_data_workspace_size(E, D, H), dev)
    _lib.call_tag[0] = {"layer": f"D{D}xH{H}", "flops": 2 * nnconv_flops(E, D, H)}
    call("mvml_nnconv_bwd_data", N, E, ptr(g.in_src), ptr(sd), ptr(g.out_rowptr), ptr(g.out_inslot), ptr(h), h.stride(0),
         D, ptr(z), z.stride(0), H, ptr(image), ptr(g_pre), D, int(accumulate), ptr(acc.dz), H, ptr(dH), D, wp, wn, st)
    if acc.weight_grad == "split_fp16":
        if acc.z_image is None:
            acc.z_image = nnconv_z_image(z, E)
        wp, wn = _lib.ws_ptr_size(L.mvml_nnconv_bwd_weight_f16x2_workspace_size(E, D, H), dev)
        _lib.call_tag[0] = {"layer": f"D{D}xH{H}", "flops": nnconv_flops(E, D, H)}
        call("mvml_nnconv_bwd_weight_f16x2", E, ptr(g.in_src), ptr(sd), ptr(h), h.stride(0), D, ptr(z), z.stride(0), H,
             ptr(g_pre), D, int(accumulate), ptr(acc.dW2), wp, wn, st, ptr(acc.z_image))
    else:
        wp, wn = _lib.ws_ptr_size(L.mvml_nnconv_bwd_weight_workspace_size(E, D, H), dev)
        _lib.call_tag[0] = {"layer": f"D{D}xH{H}", "flops": nnconv_flops(E, D, H)}
        call("mvml_nnconv_bwd_weight", E, ptr(g.in_src), ptr(sd), ptr(h), h.stride(0), D, ptr(z), z.stride(0), H, ptr(g_pre),
             D, int(accumulate), ptr(acc.dW2), wp, wn, st)
    # the b2 part, out += S view(b2): dB2 = S^T g, dS = g B2^T, dh += the sum of dS over the out-edges
    beta = 1.0 if accumulate else 0.0
    gemm(S, g_pre, D, D, N, 1, 1, D, D, acc.db2, D, beta=beta)
    if E:
        dS = torch.empty((N, D), dtype=torch.float32, device=dev)
        gemm(g_pre, b2, N, D, D, 0, 0, D, D, dS, D)
        dHb = gcn_agg(dS, D, D, g, (None, None), transpose=True)
        call("mvml_add_cols_f32", N, D, ptr(dHb), D, ptr(dH), D, st)
    colsum(g_pre, N, D, D, acc.dbias, beta=beta)
    return dH


class NNConvFunction(torch.autograd.Function):
    """act(NNConv(h)) of one message-passing step as ONE autograd node (dgl 0.9.1 NNConv.forward, sum
    aggregator; restated): mvml_nnconv_fwd for the z W2^T part of the per-edge weights, mvml_gcn_agg
    and a GEMM for the b2 part, bias and the ReLU in their epilogues.  z [E, H] is the edge network's
    hidden layer in in-CSR slot order (EdgeNetworkFunction), W2 / b2 its last Linear.  shared: the
    NNConvShared of the forward this step belongs to (None: a step of its own)."""

    @staticmethod
    def forward(ctx, h, z, W2, b2, bias, g, act, shared):
        _check_cuda_f32(h, "node_feats")
        _check_cuda_f32(z, "edge hidden rows")
        h, z, W2, b2 = _rows_f32(h), _rows_f32(z), _c(W2), _c(b2)
        N, D = h.shape
        H = z.shape[1]
        if z.shape[0] != g.num_edges() or tuple(b2.shape) != (D * D,):
            raise ValueError(f"NNConv: z must be [E = {g.num_edges()}, H] and edge_func's last bias [{D * D}] "
                             f"(got {tuple(z.shape)}, {tuple(b2.shape)})")
        image = shared.image if shared is not None else nnconv_image(W2, D, H)
        bias = None if bias is None else _c(bias)
        out, S = nnconv_forward(g, h, z, b2, bias, image, act)
        ctx.state = (g, h, z, b2, bias is not None, image, S, int(act), shared)
        ctx.save_for_backward(out)
        return out

    @staticmethod
    def backward(ctx, g_out):
        g, h, z, b2, has_bias, image, S, act, shared = ctx.state
        acc = shared if shared is not None else NNConvShared(image, 1)
        N, D = h.shape
        E, H = g.num_edges(), z.shape[1]
        first = acc.done == 0
        if first:
            acc.alloc(E, D, H, h.device)
        dH = nnconv_backward(g, h, z, b2, image, S, ctx.saved_tensors[0], g_out, act, acc, not first)
        acc.done += 1
        if acc.done < acc.steps:  # a later backward hands the sums over
            return dH, None, None, None, None, None, None, None
        acc.z_image = None
        return dH, acc.dz[:E], acc.dW2, acc.db2, acc.dbias if has_bias else None, None, None, None


class EdgeNetworkFunction(torch.autograd.Function):
    """z = ReLU(Linear1(bond rows)) [E, H] in in-CSR slot order: the bond rows permuted and padded
    to 4 columns once per batch (mvml_afp_edge_rows), then the Linear + ReLU GEMM.  Bond features
    get no gradient."""

    @staticmethod
    def forward(ctx, edge_feats, g, W1, b1):
        rows = afp_edge_rows(g, edge_feats)
        E = g.num_edges()
        H, De = W1.shape
        if edge_feats.shape[1] != De:
            raise ValueError(f"MPNN: {De} bond features expected, got {edge_feats.shape[1]}")
        ctx.De = De
        if E == 0:  # a batch without any bond: no rows, zero gradients
            ctx.state = (H, g.device)
            return torch.empty((0, H), dtype=torch.float32, device=g.device)
        Wp = zeros((H, rows.shape[1]), device=g.device)
        copy2d(Wp[:, :De], _c(W1))
        rows, Wp, z, lm = linear_forward(rows, Wp, b1, act=1)
        ctx.state = (rows, Wp, lm)
        ctx.save_for_backward(z)
        return z

    @staticmethod
    def backward(ctx, g_z):
        if len(ctx.state) == 2:
            H, dev = ctx.state
            return None, None, zeros((H, ctx.De), device=dev), zeros(H, device=dev)
        rows, Wp, lm = ctx.state
        z, = ctx.saved_tensors
        g_z = _c(g_z)
        g_pre = torch.empty_like(z)
        call("mvml_relu_bwd", z.numel(), ptr(z), ptr(g_z), ptr(g_pre), 1.0, _stream(z.device))
        _, gWp, gb = linear_backward(rows, Wp, g_pre, lm, need_gx=False)
        return None, None, _dense(gWp[:, :ctx.De]), gb


class GRUCellFunction(torch.autograd.Function):
    """torch GRUCell(x, h) as one autograd node: two gate GEMMs and mvml_gru_cell_fwd / _bwd."""

    @staticmethod
    def forward(ctx, x, h, w_ih, w_hh, b_ih, b_hh):
        _check_cuda_f32(x, "x")
        out, ctx.state = _gru_forward(x, _c(h), w_ih, w_hh, b_ih, b_hh, False)
        return out

    @staticmethod
    def backward(ctx, g_out):
        return _gru_backward(ctx.state, None, g_out)


# ---- D-MPNN: directed bond messages on csrc/dmpnn.hip ("D-MPNN") ------------------------
DMPNN_MAX_WIDTH = 1024  # hidden_size (mvml_dmpnn_update)


def dmpnn_check(who, D, De, depth):
    """What mvml_dmpnn_* take: D a positive multiple of 4 up to 1024, 1..32 bond features, depth >= 1."""
    if not isinstance(D, int) or D <= 0 or D % 4 or D > DMPNN_MAX_WIDTH:
        raise ValueError(f"{who}: hidden_size must be a positive multiple of 4, at most {DMPNN_MAX_WIDTH}, on the HIP "
                         f"path (got {D})")
    if not isinstance(De, int) or not 1 <= De <= AFP_MAX_EDGE_FEATS:
        raise ValueError(f"{who}: 1 to {AFP_MAX_EDGE_FEATS} bond features on the HIP path (got {De})")
    if not isinstance(depth, int) or depth < 1:
        raise ValueError(f"{who}: depth must be at least 1 (got {depth})")


def dmpnn_init_bytes(N, E, D, De):
    """Algorithmic HBM bytes of one mvml_dmpnn_init_fwd: P, the bond rows, the sources and W_ieT read
    once, input and M0 written (re-gathers of P rows not counted)."""
    return 4 * (N * D + E * _round4(De) + E + (De + 1) * D + 2 * E * D)


def dmpnn_update_bytes(N, E, D, backward=False):
    """Algorithmic HBM bytes of one mvml_dmpnn_update (R and input read, out written) or of its
    adjoint (out and g_out read, dR and dpre written), with both row pointers, out_inslot and the
    reverse map; the re-read of the reverse rows is not counted."""
    return 4 * ((4 if backward else 3) * E * D + 2 * (N + 1) + 2 * E + (0 if backward else D))


def dmpnn_atom_sum_bytes(N, E, D):
    """Algorithmic HBM bytes of mvml_dmpnn_atom_sum or its adjoint: the E slot rows and the N atom rows."""
    return 4 * ((N + E) * D + N + 1)


def dmpnn_rev_slots(g):
    """int32 [E]: the in-CSR slot of every slot's reverse bond, -1 for none (mvml_dmpnn_rev_slots),
    made once per batch and kept on it; BatchedMolGraph.recollate() drops it."""
    d = g._dev
    if "dmpnn_rev_slots" not in d:
        t = torch.empty(max(g.num_edges(), 1), dtype=torch.int32, device=g.device)
        call("mvml_dmpnn_rev_slots", g.num_nodes(), g.num_edges(), ptr(g.in_rowptr), ptr(g.in_src), ptr(t),
             _stream(g.device))
        d["dmpnn_rev_slots"] = t
    return d["dmpnn_rev_slots"]


def dmpnn_update(g, R, inp, b_h):
    """The next bond state [E, D] from R = M W_h^T and input (mvml_dmpnn_update); all in slot order."""
    E, D = R.shape
    out = torch.empty((E, D), dtype=torch.float32, device=R.device)
    _lib.call_tag[0] = {"layer": f"D{D}", "bytes": dmpnn_update_bytes(g.num_nodes(), E, D)}
    call("mvml_dmpnn_update", g.num_nodes(), E, ptr(g.in_rowptr), ptr(g.out_rowptr), ptr(g.out_inslot),
         ptr(dmpnn_rev_slots(g)), ptr(R), R.stride(0), ptr(inp), inp.stride(0), ptr(b_h), D, ptr(out), D, _stream(R.device))
    return out


def dmpnn_update_bwd(g, out, g_out):
    """(dR, dpre) of dmpnn_update from its output and g_out = dL/d out (mvml_dmpnn_update_bwd)."""
    E, D = out.shape
    dR, dpre = torch.empty_like(out), torch.empty_like(out)
    _lib.call_tag[0] = {"layer": f"D{D}", "bytes": dmpnn_update_bytes(g.num_nodes(), E, D, True)}
    call("mvml_dmpnn_update_bwd", g.num_nodes(), E, ptr(g.in_rowptr), ptr(g.out_rowptr), ptr(g.out_inslot),
         ptr(dmpnn_rev_slots(g)), ptr(out), out.stride(0), ptr(g_out), g_out.stride(0), D, ptr(dR), D, ptr(dpre), D,
         _stream(out.device))
    return dR, dpre


def dmpnn_atom_sum(g, M, transpose=False):
    """[N, D]: per atom the sum of its in-slot rows of M, or (transpose) of the slot rows of its
    out-edges, the adjoint of gathering an atom row per slot by in_src (mvml_dmpnn_atom_sum)."""
    N, E, D = g.num_nodes(), g.num_edges(), M.shape[1]
    a = torch.empty((N, D), dtype=torch.float32, device=M.device)
    rowptr, idx = (g.out_rowptr, g.out_inslot) if transpose else (g.in_rowptr, None)
    _lib.call_tag[0] = {"layer": f"D{D}", "bytes": dmpnn_atom_sum_bytes(N, E, D)}
    call("mvml_dmpnn_atom_sum", N, E, ptr(rowptr), ptr(idx), ptr(M), M.stride(0) if E else D, D, ptr(a), D,
         _stream(M.device))
    return a


def _dmpnn_split(W, Fa, Fp):
    """(W[:, :Fa] zero-padded to Fp columns, W[:, Fa:] dense) of a weight over [atom features ; rest]."""
    Wa = zeros((W.shape[0], Fp), device=W.device)
    copy2d(Wa[:, :Fa], W[:, :Fa])
    return Wa, _dense(W[:, Fa:])


def _dmpnn_join(ga, gb):
    """The gradient of such a weight from those of its two column blocks."""
    Fa = ga.shape[1]
    gW = torch.empty((ga.shape[0], Fa + gb.shape[1]), dtype=torch.float32, device=ga.device)
    copy2d(gW[:, :Fa], ga)
    copy2d(gW[:, Fa:], gb)
    return gW


class DMPNNInitFunction(torch.autograd.Function):
    """(input, M0) [E, D] in in-CSR slot order: input_s = W_i [x_u ; e_s] (+ b_i) for s = (u -> v), M0 =
    relu(input).  Re-associated, no [E, Fa + De] concat: P = x W_ia^T is one GEMM over the atom rows,
    mvml_dmpnn_init_fwd gathers it and adds the bond part.  The backward needs no kernel of its own:
    gP by mvml_dmpnn_atom_sum over the out-edges, the bond columns' gradient rows^T g_input on the
    GEMM.  Bond features get no gradient."""

    @staticmethod
    def forward(ctx, x, edge_feats, g, W_i, b_i):
        _check_cuda_f32(x, "node_feats")
        ctx.set_materialize_grads(False)
        X, Xp = _padded_input(x)
        N, Fa = X.shape
        D, De = W_i.shape[0], W_i.shape[1] - Fa
        E, dev = g.num_edges(), X.device
        rows = afp_edge_rows(g, edge_feats)
        if edge_feats.shape[1] != De:
            raise ValueError(f"D-MPNN: {De} bond features expected, got {edge_feats.shape[1]}")
        inp = torch.empty((E, D), dtype=torch.float32, device=dev)
        M0 = torch.empty((E, D), dtype=torch.float32, device=dev)
        ctx.dims, ctx.dev = (W_i.shape, b_i is not None, Fa), dev
        if E == 0:  # a batch without any bond: no rows, zero gradients
            ctx.state = None
            return inp, M0
        W_i = _c(W_i)
        Wa, We = _dmpnn_split(W_i, Fa, Xp.shape[1])
        Xp, Wa, P, lm = linear_forward(Xp, Wa, None)
        WieT = torch.empty((De, D), dtype=torch.float32, device=dev)
        call("mvml_transpose", D, De, ptr(We), De, ptr(WieT), D, _stream(dev))
        _lib.call_tag[0] = {"layer": f"D{D}xDe{De}", "bytes": dmpnn_init_bytes(N, E, D, De)}
        call("mvml_dmpnn_init_fwd", N, E, ptr(g.in_src), ptr(P), D, D, ptr(rows), De, ptr(WieT),
             ptr(None if b_i is None else _c(b_i)), ptr(inp), D, ptr(M0), D, _stream(dev))
        ctx.state = (g, rows, Xp, Wa, lm)
        ctx.save_for_backward(M0)
        return inp, M0

    @staticmethod
    def backward(ctx, g_inp, g_M0):
        shape, has_bias, Fa = ctx.dims
        D, De = shape[0], shape[1] - Fa
        if ctx.state is None or (g_inp is None and g_M0 is None):
            dev = ctx.dev
            return None, None, None, zeros(tuple(shape), device=dev), zeros(D, device=dev) if has_bias else None
        g, rows, Xp, Wa, lm = ctx.state
        (M0,) = ctx.saved_tensors
        E, dev = M0.shape[0], M0.device
        st = _stream(dev)
        if g_M0 is not None:  # g_in = g_input + g_M0 * (M0 > 0)
            g_in = torch.empty_like(M0)
            call("mvml_relu_bwd", M0.numel(), ptr(M0), ptr(_c(g_M0)), ptr(g_in), 1.0, st)
            if g_inp is not None:
                g_inp = _rows_f32(g_inp)
                call("mvml_add_cols_f32", E, D, ptr(g_inp), g_inp.stride(0), ptr(g_in), D, st)
        else:
            g_in = _c(g_inp)
        gP = dmpnn_atom_sum(g, g_in, transpose=True)
        gXp, gWa, _ = linear_backward(Xp, Wa, gP, lm, need_gb=False, need_gx=ctx.needs_input_grad[0])
        Dp = rows.shape[1]
        gWe = torch.empty((D, Dp), dtype=torch.float32, device=dev)
        gemm(g_in, rows, D, Dp, E, 1, 1, D, Dp, gWe, Dp)  # g_in^T rows: the bond columns
        gb = None
        if has_bias:
            gb = torch.empty(D, dtype=torch.float32, device=dev)
            colsum(g_in, E, D, D, gb)
        gX = _dense(gXp[:, :Fa]) if gXp is not None else None
        return gX, None, None, _dmpnn_join(gWa[:, :Fa], gWe[:, :De]), gb


class DMPNNStepFunction(torch.autograd.Function):
    """One depth step, M' = relu(input + W_h (sum of the bond states entering the source atom - the
    reverse bond's) (+ b_h)), as one autograd node: R = M W_h^T on the GEMM over the E slot rows (no
    gather), then mvml_dmpnn_update.  Backward: the adjoint kernel gives dR and dpre (the gradient
    of input; its column sums that of b_h), then the Linear's two products."""

    @staticmethod
    def forward(ctx, inp, M, W_h, b_h, g):
        _check_cuda_f32(M, "bond states")
        E, D = M.shape
        if E != g.num_edges() or tuple(inp.shape) != (E, D) or tuple(W_h.shape) != (D, D):
            raise ValueError(f"D-MPNN step: input and M must be [E = {g.num_edges()}, D] and W_h [D, D] "
                             f"(got {tuple(inp.shape)}, {tuple(M.shape)}, {tuple(W_h.shape)})")
        ctx.has_bias = b_h is not None
        if E == 0:
            ctx.state = None
            ctx.D = D
            return torch.empty_like(M)
        M, W_h, R, lm = linear_forward(M, W_h, None)
        out = dmpnn_update(g, R, _rows_f32(inp), None if b_h is None else _c(b_h))
        ctx.state = (g, M, W_h, lm)
        ctx.save_for_backward(out)
        return out

    @staticmethod
    def backward(ctx, g_out):
        if ctx.state is None:
            D, dev = ctx.D, g_out.device
            return g_out, g_out, zeros((D, D), device=dev), zeros(D, device=dev) if ctx.has_bias else None, None
        g, M, W_h, lm = ctx.state
        (out,) = ctx.saved_tensors
        E, D = out.shape
        dR, dpre = dmpnn_update_bwd(g, out, _rows_f32(g_out))
        gM, gW, _ = linear_backward(M, W_h, dR, lm, need_gb=False)
        gb = None
        if ctx.has_bias:
            gb = torch.empty(D, dtype=torch.float32, device=out.device)
            colsum(dpre, E, D, D, gb)
        return dpre, gM, gW, gb, None


class DMPNNOutputFunction(torch.autograd.Function):
    """h_v = relu(W_o [x_v ; a_v] + b_o), a_v = the sum of the bond states entering v
    (mvml_dmpnn_atom_sum), without the [N, Fa + D] concat: two GEMMs, the second onto the first with
    the ReLU in its epilogue."""

    @staticmethod
    def forward(ctx, x, M, g, W_o, b_o):
        _check_cuda_f32(x, "node_feats")
        X, Xp = _padded_input(x)
        N, Fa = X.shape
        W_o = _c(W_o)
        D = W_o.shape[0]
        Wa, Wm = _dmpnn_split(W_o, Fa, Xp.shape[1])
        a = dmpnn_atom_sum(g, _rows_f32(M))
        Xp, Wa, y, lmx = linear_forward(Xp, Wa, b_o)
        a, Wm, h, lma = linear_forward(a, Wm, None, act=1, onto=y)
        ctx.state = (g, Xp, Wa, lmx, a, Wm, lma, Fa)
        ctx.save_for_backward(h)
        return h

    @staticmethod
    def backward(ctx, g_h):
        g, Xp, Wa, lmx, a, Wm, lma, Fa = ctx.state
        (h,) = ctx.saved_tensors
        N, D = h.shape
        E, dev = g.num_edges(), h.device
        g_pre = torch.empty_like(h)
        call("mvml_relu_bwd", h.numel(), ptr(h), ptr(_c(g_h)), ptr(g_pre), 1.0, _stream(dev))
        g_a, gWm, _ = linear_backward(a, Wm, g_pre, lma, need_gb=False)
        gXp, gWa, gb = linear_backward(Xp, Wa, g_pre, lmx, need_gx=ctx.needs_input_grad[0])
        gM = torch.empty((E, D), dtype=torch.float32, device=dev)
        _lib.call_tag[0] = {"layer": f"D{D}", "bytes": dmpnn_atom_sum_bytes(N, E, D)}
        call("mvml_dmpnn_atom_sum_bwd", N, E, ptr(g.in_rowptr), ptr(g_a), D, D, ptr(gM), D, _stream(dev))
        gX = _dense(gXp[:, :Fa]) if gXp is not None else None
        return gX, gM, None, _dmpnn_join(gWa[:, :Fa], gWm), gb


# ---- SchNet: the fused filter network and CFConv on csrc/schnet.hip ("SchNet") ----------
SCHNET_MAX_H = 128     # hidden_feats of a CFConv (mvml_schnet_filter_fwd)
SCHNET_MAX_K = 512     # radial-basis centres
SCHNET_MAX_F = 1024    # node_feats


def schnet_num_centers(cutoff, gap):
    """K = ceil(cutoff / gap), dgllife's RBFExpansion count; ValueError naming the argument at fault."""
    if not cutoff > 0:
        raise ValueError(f"SchNet: cutoff must be positive (got {cutoff})")
    if not gap > 0:
        raise ValueError(f"SchNet: gap must be positive (got {gap})")
    K = int(np.ceil(cutoff / gap))
    if not 1 <= K <= SCHNET_MAX_K:
        raise ValueError(f"SchNet: cutoff / gap must give 1 to {SCHNET_MAX_K} centres on the HIP path (got K = {K})")
    return K


def schnet_check(who, F=None, H=None):
    """The widths mvml_schnet_* take: hidden_feats a multiple of 16 in [16, 128], node_feats a
    positive multiple of 4 up to 1024."""
    if H is not None and (not isinstance(H, int) or H < 16 or H % 16 or H > SCHNET_MAX_H):
        raise ValueError(f"{who}: hidden_feats must be a multiple of 16 in [16, {SCHNET_MAX_H}] on the HIP path (got {H})")
    if F is not None and (not isinstance(F, int) or F <= 0 or F % 4 or F > SCHNET_MAX_F):
        raise ValueError(f"{who}: node_feats must be a positive multiple of 4, at most {SCHNET_MAX_F}, on the HIP path "
                         f"(got {F})")


def schnet_filter_flops(E, H, K):
    """Useful flops of one filter forward: the K x H and the H x H product per edge (the MFMA work is
    three times that, before K's padding to a multiple of 32)."""
    return 2 * E * H * (K + H)


def schnet_filter_fwd_bytes(E, H, K):
    """Algorithmic HBM bytes of one mvml_schnet_filter_fwd: one float per edge read, s1 and he written;
    the centres, biases and the three-image weight file once."""
    return 4 * (E + 2 * E * H + K + 2 * H) + _lib.lib().mvml_schnet_image_bytes(H, K)


def schnet_filter_bwd_bytes(N, E, H):
    """Algorithmic bytes of one mvml_schnet_filter_bwd: he and s1 read, dpre2 and dpre1 written, both
    index lists, the dA and hv rows once (re-gathers not counted), W_2's transposed image."""
    return 4 * (4 * E * H + 2 * E + 2 * N * H) + 2 * H * H * 4


def schnet_dw1_bytes(E, H, K):
    """Algorithmic bytes of one mvml_schnet_dw1: dpre1 once per group of 64 centres, one float per edge,
    the partials written and re-read, dW_1."""
    S = max(1, min(-(-E // 128), 128))
    return 4 * (-(-K // 64) * E * H + E + 2 * S * H * K + H * K)


def cfconv_agg_bytes(N, E, H):
    """Algorithmic bytes of one mvml_cfconv_agg: the E filter rows and the N atom rows read once
    (re-gathers not counted), out written, the row pointers and up to two index lists."""
    return 4 * (E * H + 2 * N * H + N + 1 + 2 * E)


def schnet_slot_dists(g, edge_dists):
    """(d, stride): the distances in in-CSR slot order, column 0 of the padded rows of
    mvml_afp_edge_rows; permuted once per (batch, tensor), kept on the batch and dropped by
    BatchedMolGraph.recollate()."""
    E = g.num_edges()
    d = edge_dists
    if d.dim() == 1:
        d = d.view(-1, 1)
    if d.dim() != 2 or tuple(d.shape) != (E, 1):
        raise ValueError(f"edge_dists: a float [E = {E}] or [E, 1] tensor in edge-id order expected, got "
                         f"{tuple(edge_dists.shape)}")
    rows = afp_edge_rows(g, d)
    return rows, rows.shape[1]


def schnet_image(W1, W2, H, K):
    """max |W_1|, max |W_2| and the split-fp16 images of W_1, W_2 and W_2^T (mvml_schnet_split_w)."""
    nbytes = _lib.lib().mvml_schnet_image_bytes(H, K)
    if nbytes == 0 or tuple(W1.shape) != (H, K) or tuple(W2.shape) != (H, H):
        raise ValueError(f"CFConv: project_edge must be Linear({K}, {H}), Linear({H}, {H}) with H a multiple of 16 <= "
                         f"{SCHNET_MAX_H} and K <= {SCHNET_MAX_K} (weights {tuple(W1.shape)}, {tuple(W2.shape)})")
    img = torch.empty(nbytes, dtype=torch.uint8, device=W1.device)
    call("mvml_schnet_split_w", H, K, ptr(W1), ptr(W2), ptr(img), _stream(W1.device))
    return img


def schnet_dw1(dists, ldd, centers, gamma, dpre1, E, H, K, out, accumulate=False):
    """out [H, K] (+)= dpre1^T rbf(dists) with the expansion generated in the kernel (mvml_schnet_dw1)."""
    wp, wn = _lib.ws_ptr_size(_lib.lib().mvml_schnet_dw1_workspace_size(E, H, K), out.device)
    _lib.call_tag[0] = {"layer": f"H{H}xK{K}", "flops": 2 * E * H * K, "bytes": schnet_dw1_bytes(E, H, K)}
    call("mvml_schnet_dw1", E, ptr(dists), ldd, ptr(centers), K, float(gamma), ptr(dpre1), H, H, int(accumulate), ptr(out),
         wp, wn, _stream(out.device))
    return out


def cfconv_agg(g, X, he, transpose=False):
    """[N, H]: a_v = sum over v's in-slots s of X[src s] * he[s], or (transpose) the gradient of the
    gathered rows, sum over u's out-edges of X[dst s] * he[s] (mvml_cfconv_agg; he in slot order)."""
    N, E, H = g.num_nodes(), g.num_edges(), X.shape[1]
    out = torch.empty((N, H), dtype=torch.float32, device=X.device)
    rowptr, widx, xidx = (g.out_rowptr, g.out_inslot, nnconv_slot_dst(g)) if transpose else (g.in_rowptr, None, g.in_src)
    _lib.call_tag[0] = {"layer": f"H{H}", "bytes": cfconv_agg_bytes(N, E, H)}
    call("mvml_cfconv_agg", N, E, ptr(rowptr), ptr(widx), ptr(xidx), ptr(X), X.stride(0), ptr(he), he.stride(0) if E else H,
         H, ptr(out), H, _stream(X.device))
    return out


class CFConvLink:
    """What joins a layer's CFConvAggFunction to its SchNetFilterFunction in the backward: the
    gradient of he, dA[dst] * hv[src], is never written; the aggregation's backward leaves dA and hv
    here and mvml_schnet_filter_bwd forms the product as it loads."""
    dA = hv = None


class SchNetFilterFunction(torch.autograd.Function):
    """he = ssp(ssp(rbf(d) W_1^T + b_1) W_2^T + b_2) [E, H] in in-CSR slot order from the distances
    (edge-id order), as ONE autograd node with the four parameters as leaves: mvml_schnet_split_w once
    per call, then mvml_schnet_filter_fwd; the [E, K] expansion does not exist.  link: the CFConvLink
    shared with the CFConvAggFunction that consumes he; the backward takes dA and hv from it (the
    gradient autograd hands over for he is a placeholder without storage), runs
    mvml_schnet_filter_bwd and mvml_schnet_dw1, dW_2 on the k-major GEMM and both bias gradients on
    mvml_colsum_f32.  Distances and centres get no gradient."""

    @staticmethod
    def forward(ctx, edge_dists, centers, gamma, W1, b1, W2, b2, g, link):
        _check_cuda_f32(edge_dists, "edge_dists")
        for t in (centers, W1, b1, W2, b2):
            _check_cuda_f32(t, "CFConv parameters")
        H, K = W1.shape
        E, dev = g.num_edges(), g.device
        centers, W1, b1, W2, b2 = _c(centers), _c(W1), _c(b1), _c(W2), _c(b2)
        if centers.numel() != K:
            raise ValueError(f"CFConv: {K} centres expected by project_edge, the expansion has {centers.numel()}")
        image = schnet_image(W1, W2, H, K)
        d, ldd = schnet_slot_dists(g, edge_dists)
        s1 = torch.empty((E, H), dtype=torch.float32, device=dev)
        he = torch.empty((E, H), dtype=torch.float32, device=dev)
        _lib.call_tag[0] = {"layer": f"H{H}xK{K}", "flops": schnet_filter_flops(E, H, K),
                            "bytes": schnet_filter_fwd_bytes(E, H, K)}
        call("mvml_schnet_filter_fwd", E, ptr(d), ldd, ptr(centers), K, float(gamma), H, ptr(image), ptr(b1), ptr(b2),
             ptr(s1), H, ptr(he), H, _stream(dev))
        ctx.state = (g, d, ldd, centers, float(gamma), image, link, H, K)
        ctx.save_for_backward(s1, he)
        return he

    @staticmethod
    def backward(ctx, _g_he):
        g, d, ldd, centers, gamma, image, link, H, K = ctx.state
        s1, he = ctx.saved_tensors
        N, E, dev = g.num_nodes(), g.num_edges(), g.device
        f32 = dict(dtype=torch.float32, device=dev)
        if link is None or link.dA is None:
            raise RuntimeError("SchNetFilterFunction: he must be consumed by a CFConvAggFunction that shares its link")
        dA, hv = link.dA, link.hv
        link.dA = link.hv = None
        if E == 0:  # a batch without any bond: no rows, zero gradients
            return (None, None, None, zeros((H, K), device=dev), zeros(H, device=dev), zeros((H, H), device=dev),
                    zeros(H, device=dev), None, None)
        dpre2, dpre1 = torch.empty((E, H), **f32), torch.empty((E, H), **f32)
        _lib.call_tag[0] = {"layer": f"H{H}", "flops": 2 * E * H * H, "bytes": schnet_filter_bwd_bytes(N, E, H)}
        call("mvml_schnet_filter_bwd", E, ptr(g.in_src), ptr(nnconv_slot_dst(g)), ptr(dA), dA.stride(0), ptr(hv),
             hv.stride(0), ptr(s1), H, ptr(he), H, H, K, ptr(image), ptr(dpre2), H, ptr(dpre1), H, _stream(dev))
        dW2 = torch.empty((H, H), **f32)
        gemm(dpre2, s1, H, H, E, 1, 1, H, H, dW2, H)  # dpre2^T s1
        db2, db1 = torch.empty(H, **f32), torch.empty(H, **f32)
        colsum(dpre2, E, H, H, db2)
        colsum(dpre1, E, H, H, db1)
        dW1 = schnet_dw1(d, ldd, centers, gamma, dpre1, E, H, K, torch.empty((H, K), **f32))
        return None, None, None, dW1, db1, dW2, db2, None, None


class CFConvAggFunction(torch.autograd.Function):
    """a_v = sum_{u -> v} hv[u] * he_s (dgl's u_mul_e, sum) with he [E, H] in slot order
    (mvml_cfconv_agg).  Backward: dL/dhv by the same kernel over the out-edges; dA and hv go to link
    for SchNetFilterFunction, and he's gradient is a placeholder without storage (a zero expanded to
    [E, H]): its rows exist only inside mvml_schnet_filter_bwd.  Without a link he gets no gradient."""

    @staticmethod
    def forward(ctx, hv, he, g, link):
        _check_cuda_f32(hv, "node rows")
        _check_cuda_f32(he, "filter rows")
        hv, he = _rows_f32(hv), _rows_f32(he)
        if he.shape[0] != g.num_edges() or he.shape[1] != hv.shape[1] or hv.shape[0] != g.num_nodes():
            raise ValueError(f"CFConv: hv must be [N = {g.num_nodes()}, H] and he [E = {g.num_edges()}, H] "
                             f"(got {tuple(hv.shape)}, {tuple(he.shape)})")
        ctx.state = (g, hv, he, link)
        return cfconv_agg(g, hv, he)

    @staticmethod
    def backward(ctx, g_a):
        g, hv, he, link = ctx.state
        dA = _rows_f32(g_a)
        d_hv = cfconv_agg(g, dA, he, transpose=True)
        if link is None:
            return d_hv, None, None, None
        link.dA, link.hv = dA, hv
        return d_hv, dA.new_zeros(()).expand(he.shape), None, None


class LinearSSPFunction(torch.autograd.Function):
    """ssp(x W^T + b), ssp = softplus - ln 2: the GEMM with its bias epilogue, mvml_ssp_fwd in place;
    the backward takes ssp' from the output (mvml_ssp_bwd) and runs the Linear's three products."""

    @staticmethod
    def forward(ctx, x, weight, bias):
        _check_cuda_f32(x, "x")
        x, weight, y, ctx.lm = linear_forward(x, weight, bias)
        call("mvml_ssp_fwd", y.numel(), ptr(y), ptr(y), _stream(y.device))
        ctx.save_for_backward(x, weight, y)
        return y

    @staticmethod
    def backward(ctx, g_y):
        x, weight, y = ctx.saved_tensors
        g_pre = torch.empty_like(y)
        call("mvml_ssp_bwd", y.numel(), ptr(y), ptr(_c(g_y)), ptr(g_pre), _stream(y.device))
        return linear_backward(x, weight, g_pre, ctx.lm, need_gx=ctx.needs_input_grad[0])


class SSPFunction(torch.autograd.Function):
    """ssp(x) = softplus(x) - ln 2 element-wise (mvml_ssp_fwd / mvml_ssp_bwd, the backward from the output)."""

    @staticmethod
    def forward(ctx, x):
        _check_cuda_f32(x, "x")
        y = torch.empty_like(_c(x))
        call("mvml_ssp_fwd", y.numel(), ptr(_c(x)), ptr(y), _stream(y.device))
        ctx.save_for_backward(y)
        return y

    @staticmethod
    def backward(ctx, g_y):
        (y,) = ctx.saved_tensors
        g_x = torch.empty_like(y)
        call("mvml_ssp_bwd", y.numel(), ptr(y), ptr(_c(g_y)), ptr(g_x), _stream(y.device))
        return g_x


class NodeReadoutFunction(torch.autograd.Function):
    """The per-molecule pool of (h W^T + b) [N, T] for any T >= 1 (MLPNodeReadout's out_project, T =
    n_tasks): mvml_segment_pool_* walks float4 columns, so W and b are zero-padded to a multiple of 4
    rows for the GEMM and the pool, and the [B, T] block is copied out (mvml_copy_cols)."""

    @staticmethod
    def forward(ctx, h, weight, bias, g, mode):
        _check_cuda_f32(h, "node rows")
        T, K = weight.shape
        Tp, dev = _round4(T), h.device
        Wp, bp = zeros((Tp, K), device=dev), zeros(Tp, device=dev)
        copy2d(Wp[:T], _c(weight))
        copy2d(bp[:T], _c(bias))
        h, Wp, rows, lm = linear_forward(h, Wp, bp)
        ctx.pool = _StageCtx()
        pooled = SegmentPoolFunction.forward(ctx.pool, rows, g, mode)
        ctx.state = (h, Wp, lm, T)
        return _dense(pooled[:, :T])

    @staticmethod
    def backward(ctx, g_out):
        h, Wp, lm, T = ctx.state
        Gp = zeros((g_out.shape[0], Wp.shape[0]), device=h.device)
        copy2d(Gp[:, :T], _c(g_out))
        g_rows = SegmentPoolFunction.backward(ctx.pool, Gp)[0]
        gx, gWp, gbp = linear_backward(h, Wp, g_rows, lm, need_gx=ctx.needs_input_grad[0])
        return gx, _dense(gWp[:T]), _dense(gbp[:T]), None, None


# ---- Weave: the Gaussian-histogram readout on csrc/weave_gather.hip ("Weave") -----------
WEAVE_MAX_MEMBERSHIPS = 16  # mvml_weave_gather_fwd
WEAVE_MAX_GATHER_F = 1024
# dgllife's default memberships (mean, std)
WEAVE_MEMBERSHIPS = ((-1.645, 0.283), (-1.080, 0.170), (-0.739, 0.134), (-0.468, 0.118), (-0.228, 0.114), (0., 0.114),
                     (0.228, 0.114), (0.468, 0.118), (0.739, 0.134), (1.080, 0.170), (1.645, 0.283))


def weave_gather_check(who, F, memberships=None):
    """What mvml_weave_gather_* take: F a multiple of 4 in [4, 1024]; 1 to 16 memberships, every mean
    finite and every std > 0."""
    if not isinstance(F, int) or F < 4 or F % 4 or F > WEAVE_MAX_GATHER_F:
        raise ValueError(f"{who}: node_in_feats must be a multiple of 4 in [4, {WEAVE_MAX_GATHER_F}] on the HIP path (got {F})")
    if memberships is None:
        return
    if not 1 <= len(memberships) <= WEAVE_MAX_MEMBERSHIPS:
        raise ValueError(f"{who}: 1 to {WEAVE_MAX_MEMBERSHIPS} gaussian memberships on the HIP path (got {len(memberships)})")
    for mean, std in memberships:
        if not (np.isfinite(mean) and np.isfinite(std) and std > 0 and np.isfinite(np.float32(1) / np.float32(std) ** 2)):
            raise ValueError(f"{who}: every membership needs a finite mean and a std > 0 (got ({mean}, {std}))")


def weave_gather_bytes(B, N, F, K):
    """Algorithmic bytes of one mvml_weave_gather_fwd: the [N, F] rows once, the [B, F K] rows once, the
    offsets.  The backward reads both and writes [N, F] more."""
    return 4 * (N * F + B * F * K) + 8 * (B + 1)


def weave_gather_exps(N, F, K):
    """exp evaluations of one mvml_weave_gather_fwd or _bwd (the backward recomputes them)."""
    return N * F * K


def _host_floats(vals):
    return (ctypes.c_float * len(vals))(*vals)


class WeaveGatherFunction(torch.autograd.Function):
    """WeaveGather's histogram and node sum as one node: out[g, f K + k] = sum over g's atoms of
    p_k(X[n, f]) (mvml_weave_gather_fwd / _bwd); [N, F K] is never formed.  means, stds: K host floats
    each (they take no gradient).  Returns (B, F K)."""

    @staticmethod
    def forward(ctx, X, g, means, stds):
        _check_cuda_f32(X, "node_feats")
        X = _rows_f32(X)
        (N, F), K, B, dev = X.shape, len(means), g.batch_size, X.device
        weave_gather_check("WeaveGatherFunction", F, list(zip(means, stds)))
        mu, sd = _host_floats(means), _host_floats(stds)
        out = torch.empty((B, F * K), dtype=torch.float32, device=dev)
        _lib.call_tag[0] = {"layer": f"F{F}xK{K}", "bytes": weave_gather_bytes(B, N, F, K)}
        call("mvml_weave_gather_fwd", B, N, F, K, mu, sd, ptr(g.node_offsets), ptr(X), X.stride(0), ptr(out), F * K, _stream(dev))
        ctx.save_for_backward(X)
        ctx.state = (g, mu, sd, K)
        return out

    @staticmethod
    def backward(ctx, g_out):
        (X,) = ctx.saved_tensors
        g, mu, sd, K = ctx.state
        G = _rows_f32(g_out)
        N, F = X.shape
        B = g.batch_size
        # (rows of atoms outside every molecule cannot exist: node_offsets covers [0, N))
        gX = torch.empty((N, F), dtype=torch.float32, device=X.device)
        _lib.call_tag[0] = {"layer": f"F{F}xK{K}", "bytes": weave_gather_bytes(B, N, F, K) + 4 * N * F}
        call("mvml_weave_gather_bwd", B, N, F, K, mu, sd, ptr(g.node_offsets), ptr(X), X.stride(0), ptr(G), G.stride(0),
             ptr(gX), F, _stream(X.device))
        return gX, None, None, None


class LinearTanhFunction(torch.autograd.Function):
    """tanh(x W^T + b): the GEMM with its bias epilogue, mvml_tanh_fwd in place; the backward takes
    1 - y^2 from the output (mvml_tanh_bwd) and runs the Linear's three products."""

    @staticmethod
    def forward(ctx, x, weight, bias):
        _check_cuda_f32(x, "x")
        x, weight, y, ctx.lm = linear_forward(x, weight, bias)
        call("mvml_tanh_fwd", y.numel(), ptr(y), ptr(y), _stream(y.device))
        ctx.save_for_backward(x, weight, y)
        return y

    @staticmethod
    def backward(ctx, g_y):
        x, weight, y = ctx.saved_tensors
        g_pre = torch.empty_like(y)
        call("mvml_tanh_bwd", y.numel(), ptr(y), ptr(_c(g_y)), ptr(g_pre), _stream(y.device))
        return linear_backward(x, weight, g_pre, ctx.lm, need_gx=ctx.needs_input_grad[0])


# ---- Weave: the pair-update layer on csrc/weave_pair.hip ("Weave: the pair update") -----
WEAVE_MAX_WIDTH = 128  # every width of mvml_weave_edge_* / mvml_weave_e2n_*
WEAVE_WIDTHS = ("node_node_hidden_feats", "edge_node_hidden_feats", "node_out_feats", "node_edge_hidden_feats",
                "edge_edge_hidden_feats", "edge_out_feats")


def weave_check(who, node_in_feats, edge_in_feats, widths, slot_input=False):
    """What a WeaveLayer takes on the HIP path: every hidden and output width and a slot-order edge input in
    [1, 128]; a user's edge_in_feats (edge-id order, through mvml_afp_edge_rows) in [1, 32]."""
    for name, w in zip(WEAVE_WIDTHS, widths):
        if not isinstance(w, int) or not 1 <= w <= WEAVE_MAX_WIDTH:
            raise ValueError(f"{who}: {name} must be in [1, {WEAVE_MAX_WIDTH}] on the HIP path (got {w})")
    hi = WEAVE_MAX_WIDTH if slot_input else AFP_MAX_EDGE_FEATS
    if not isinstance(edge_in_feats, int) or not 1 <= edge_in_feats <= hi:
        raise ValueError(f"{who}: edge_in_feats must be in [1, {hi}] on the HIP path (got {edge_in_feats})")
    if not isinstance(node_in_feats, int) or node_in_feats < 1:
        raise ValueError(f"{who}: node_in_feats must be positive (got {node_in_feats})")


def weave_edge_flops(E, De, Hne, Hee, Heo):
    """Useful flops of one mvml_weave_edge_fwd: the two products per edge (the MFMA work is three times
    that, before the padding of K to 32s and of N to 16s); the backward's are 2 E Heo (Hne + Hee)."""
    return 2 * E * (De * Hee + (Hne + Hee) * Heo)


def weave_edge_fwd_bytes(N, E, De, Hne, Hee, Heo, grad=False):
    """Algorithmic bytes of one mvml_weave_edge_fwd: e read, e' written (and the [pair | third] operand when
    a gradient is wanted), both index lists, the LR rows once (re-gathers not counted), the three images."""
    return 4 * (E * (De + Heo + (Hne + Hee if grad else 0) + 2) + 2 * N * Hne + De * Hee + (Hne + Hee) * Heo)


def weave_edge_bwd_bytes(N, E, Hne, Hee, Heo):
    """Algorithmic bytes of one mvml_weave_edge_bwd: g, e' and third read, dpre, dfirst, dsecond and dthird
    written, both index lists, the LR rows once, the transposed images."""
    return 4 * (E * (3 * Heo + 2 * Hee + 2 * Hne + 2) + 2 * N * Hne + (Hne + Hee) * Heo)


def weave_e2n_flops(E, De, Hen):
    return 2 * E * De * Hen


def weave_e2n_bytes(N, E, De, Hen, backward=False):
    """Algorithmic bytes of mvml_weave_e2n_fwd (e read, S written, the destinations) or _bwd (e and dS read,
    dpre written)."""
    return 4 * (E * (De + 1 + (Hen if backward else 0)) + N * (Hen + 1) + De * Hen)


def weave_image(De, Hee, Hen, Hne, Heo, W_ee, W_en, W_ue):
    """The maxima and split-fp16 images of a layer's three edge-side weights (mvml_weave_split_w); W_ee and
    W_ue None: a node-only layer's."""
    nbytes = _lib.lib().mvml_weave_image_bytes(De, Hee, Hen, Hne, Heo)
    if nbytes == 0:
        raise ValueError(f"WeaveLayer: every width must be in [1, {WEAVE_MAX_WIDTH}] (got {(De, Hee, Hen, Hne, Heo)})")
    img = torch.empty(nbytes, dtype=torch.uint8, device=W_en.device)
    call("mvml_weave_split_w", De, Hee, Hen, Hne, Heo, ptr(W_ee), ptr(W_en), ptr(W_ue), ptr(img), _stream(W_en.device))
    return img


def weave_permute_rows(g, rows, cols, to_edges):
    """[E, cols] dense: slot-order rows in edge-id order (to_edges) or the reverse (mvml_weave_permute_rows)."""
    E = g.num_edges()
    out = torch.empty((E, cols), dtype=torch.float32, device=rows.device)
    call("mvml_weave_permute_rows", E, cols, ptr(g.in_eid), ptr(rows), rows.stride(0) if E else cols, ptr(out), cols,
         int(to_edges), _stream(rows.device))
    return out


class WeaveEdgeOrderFunction(torch.autograd.Function):
    """Slot-order edge rows in edge-id order (what a WeaveLayer hands back to its caller); the backward is
    the reverse permutation."""

    @staticmethod
    def forward(ctx, rows, g):
        ctx.g = g
        return weave_permute_rows(g, _rows_f32(rows), rows.shape[1], True)

    @staticmethod
    def backward(ctx, g_out):
        return weave_permute_rows(ctx.g, _rows_f32(g_out), g_out.shape[1], False), None


def _rows4(t):
    """t as rows the pair-update kernels read in place (_rows_f32), else a copy at a pitch rounded up to a
    multiple of 4 (mvml_copy_cols); the pad columns are never used."""
    r = _rows_f32(t)
    if r.shape[0] == 0 or (r.stride(0) % 4 == 0 and r.data_ptr() % 16 == 0):
        return r
    buf = torch.empty((r.shape[0], _round4(r.shape[1])), dtype=torch.float32, device=r.device)
    copy2d(buf[:, :r.shape[1]], r)
    return buf[:, :r.shape[1]]


def _relu_bwd(y, g_y):
    g_x = torch.empty_like(y)
    call("mvml_relu_bwd", y.numel(), ptr(y), ptr(_c(g_y)), ptr(g_x), 1.0, _stream(y.device))
    return g_x


class WeaveLayerFunction(torch.autograd.Function):
    """One WeaveLayer as ONE autograd node with its fourteen parameters as leaves; returns (x', e') with e'
    [E, edge_out] in in-CSR slot order (None with node_only).  slot_in: edge_feats are already in slot
    order (a previous layer's e'), else in edge-id order and brought over once by mvml_afp_edge_rows.
    Node side on the GEMM: relu(node_to_node(x)); S = the destination sums of relu(edge_to_node(e))
    (mvml_weave_e2n_fwd, no [E, H] array); update_node without its concat, as two products, the second onto
    the first with the ReLU in its epilogue.  Edge side: LR = x [W_left ; W_right]^T in one product (each
    half padded to a multiple of 4 rows), then mvml_weave_edge_fwd.  Backward: mvml_weave_edge_bwd, the
    weight and bias gradients on the GEMM and mvml_colsum_f32, dLR as two mvml_dmpnn_atom_sum calls (over the
    in-slots the halves land swapped), mvml_weave_e2n_bwd, then the node side's Linears.  With node_only
    the four edge-side Linears get no gradient."""

    @staticmethod
    def forward(ctx, x, e, g, node_only, slot_in, W_nn, b_nn, W_en, b_en, W_un, b_un, W_l, b_l, W_r, b_r, W_ee, b_ee,
                W_ue, b_ue):
        _check_cuda_f32(x, "node_feats")
        _check_cuda_f32(e, "edge_feats")
        N, E, dev = g.num_nodes(), g.num_edges(), x.device
        if x.dim() != 2 or x.shape[0] != N or x.shape[1] != W_nn.shape[1]:
            raise ValueError(f"WeaveLayer: node_feats must be [N = {N}, {W_nn.shape[1]}] (got {tuple(x.shape)})")
        De = W_en.shape[1]
        if e.dim() != 2 or tuple(e.shape) != (E, De):
            raise ValueError(f"WeaveLayer: edge_feats must be [E = {E}, {De}] (got {tuple(e.shape)})")
        Hnn, Hen, Hne, Hee, Heo = W_nn.shape[0], W_en.shape[0], W_l.shape[0], W_ee.shape[0], W_ue.shape[0]
        erows = _rows4(e) if slot_in else afp_edge_rows(g, e)
        lde = erows.stride(0) if E else _round4(De)
        W_en, b_en, W_ee, b_ee, W_ue, b_ue = (_c(t) for t in (W_en, b_en, W_ee, b_ee, W_ue, b_ue))
        image = weave_image(De, Hee, Hen, Hne, Heo, None if node_only else W_ee, W_en, None if node_only else W_ue)
        dims = (De, Hee, Hen, Hne, Heo)
        st = _stream(dev)
        # node side
        x, W_nn, hn, lm_nn = linear_forward(x, W_nn, b_nn, act=1)
        S = torch.empty((N, Hen), dtype=torch.float32, device=dev)
        wp, wn = _lib.ws_ptr_size(_lib.lib().mvml_weave_e2n_workspace_size(E, Hen), dev)
        _lib.call_tag[0] = {"layer": f"De{De}xH{Hen}", "flops": weave_e2n_flops(E, De, Hen),
                            "bytes": weave_e2n_bytes(N, E, De, Hen)}
        call("mvml_weave_e2n_fwd", N, E, ptr(g.in_rowptr), ptr(nnconv_slot_dst(g)), ptr(erows), lde, De, Hee, Hen, Hne, Heo,
             ptr(image), ptr(b_en), ptr(S), Hen, wp, wn, st)
        W_un = _c(W_un)
        WunN, WunS = _dense(W_un[:, :Hnn]), _dense(W_un[:, Hnn:])
        hn, WunN, y, lmN = linear_forward(hn, WunN, b_un)
        S, WunS, xn, lmS = linear_forward(S, WunS, None, act=1, onto=y)
        ctx.dims, ctx.node_only, ctx.slot_in = dims, node_only, slot_in
        # (the outputs and the large rows go through save_for_backward, not into the node's own state)
        ctx.node = (g, W_nn, lm_nn, WunN, lmN, WunS, lmS, lde, image, W_en, b_en)
        ctx.edge = None
        if node_only:
            ctx.save_for_backward(xn, x, hn, S, erows)
            return xn, None
        # edge side.  The stacked [W_left ; W_right], like update_node's two column blocks and the weight
        # images above, is rebuilt on every call by design: a handful of small launches per layer, which
        # keeps the parameters the only state between steps (it shows on small batches only).
        Hq = _round4(Hne)
        Wlr, blr = zeros((2 * Hq, x.shape[1]), device=dev), zeros(2 * Hq, device=dev)
        for off, W, b in ((0, W_l, b_l), (Hq, W_r, b_r)):
            copy2d(Wlr[off:off + Hne], _c(W))
            copy2d(blr[off:off + Hne], _c(b))
        x, Wlr, LR, lm_lr = linear_forward(x, Wlr, blr)
        Ho4, lda = _round4(Heo), Hq + _round4(Hee)
        en = torch.empty((E, Ho4), dtype=torch.float32, device=dev)
        A = torch.empty((E, lda), dtype=torch.float32, device=dev) if any(ctx.needs_input_grad) else None
        if E:
            _lib.call_tag[0] = {"layer": f"De{De}xH{Heo}", "flops": weave_edge_flops(E, De, Hne, Hee, Heo),
                                "bytes": weave_edge_fwd_bytes(N, E, De, Hne, Hee, Heo, A is not None)}
            call("mvml_weave_edge_fwd", N, E, ptr(g.in_src), ptr(nnconv_slot_dst(g)), ptr(erows), lde, De, ptr(LR), 2 * Hq, Hq,
                 Hne, Hee, Hen, Heo, ptr(image), ptr(b_ee), ptr(b_ue), ptr(en), Ho4, ptr(A), lda, st)
        ctx.edge = (Wlr, lm_lr, W_ee, W_ue)
        en = en[:, :Heo]
        ctx.save_for_backward(xn, x, hn, S, erows, en, LR, A)
        return xn, en

    @staticmethod
    def backward(ctx, g_xn, g_en):
        g, W_nn, lm_nn, WunN, lmN, WunS, lmS, lde, image, W_en, b_en = ctx.node
        xn, x, hn, S, erows = ctx.saved_tensors[:5]
        De, Hee, Hen, Hne, Heo = ctx.dims
        N, E, dev = g.num_nodes(), g.num_edges(), x.device
        f32 = dict(dtype=torch.float32, device=dev)
        st = _stream(dev)
        need_gx, need_ge = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        De4 = _round4(De)
        de = torch.empty((E, De4), **f32) if need_ge else None
        # node side down to dS and the node_to_node branch
        g_pre = _relu_bwd(xn, g_xn)
        dS, gWunS, _ = linear_backward(S, WunS, g_pre, lmS, need_gb=False)
        dhn, gWunN, gb_un = linear_backward(hn, WunN, g_pre, lmN)
        gx, gW_nn, gb_nn = linear_backward(x, W_nn, _relu_bwd(hn, dhn), lm_nn, need_gx=need_gx)
        gW_un = _dmpnn_join(gWunN, gWunS)
        new = (lambda shape: torch.empty(shape, **f32)) if E else (lambda shape: zeros(shape, device=dev))  # (no edge: zeros)
        gW_en, gb_en = new((Hen, De)), new(Hen)
        if E:
            ldd = _round4(Hen)
            dpre_en = torch.empty((E, ldd), **f32)
            _lib.call_tag[0] = {"layer": f"De{De}xH{Hen}", "flops": weave_e2n_flops(E, De, Hen),
                                "bytes": weave_e2n_bytes(N, E, De, Hen, True)}
            call("mvml_weave_e2n_bwd", N, E, ptr(nnconv_slot_dst(g)), ptr(erows), lde, De, Hee, Hen, Hne, Heo, ptr(image),
                 ptr(b_en), ptr(dS), Hen, ptr(dpre_en), ldd, st)
            gemm(dpre_en, erows, Hen, De, E, 1, 1, ldd, lde, gW_en, De)  # dpre_en^T e
            colsum(dpre_en, E, Hen, ldd, gb_en)
            if need_ge:
                gemm(dpre_en, W_en, E, De, Hen, 0, 1, ldd, De, de, De4)
        edge_grads = (None,) * 8
        if ctx.edge is not None:
            Wlr, lm_lr, W_ee, W_ue = ctx.edge
            en, LR, A = ctx.saved_tensors[5:]  # (en: the [:, :Heo] view of its [E, Ho4] rows)
            Hq, Ho4, He4 = _round4(Hne), _round4(Heo), _round4(Hee)
            lda = Hq + He4
            gW_ue, gb_ue, gW_ee, gb_ee = new((Heo, Hne + Hee)), new(Heo), new((Hee, De)), new(Hee)
            dfs = torch.empty((E, 2 * Hq), **f32)
            if E:
                G = _rows4(g_en)
                dpre, dthird = torch.empty((E, Ho4), **f32), torch.empty((E, He4), **f32)
                _lib.call_tag[0] = {"layer": f"De{De}xH{Heo}", "flops": 2 * E * Heo * (Hne + Hee),
                                    "bytes": weave_edge_bwd_bytes(N, E, Hne, Hee, Heo)}
                call("mvml_weave_edge_bwd", N, E, ptr(g.in_src), ptr(nnconv_slot_dst(g)), ptr(G), G.stride(0), ptr(en), Ho4,
                     ptr(A), lda, ptr(LR), 2 * Hq, Hq, De, Hne, Hee, Hen, Heo, ptr(image), ptr(dpre), Ho4, ptr(dfs), 2 * Hq,
                     ptr(dthird), He4, st)
                gA = torch.empty((Heo, lda), **f32)
                gemm(dpre, A, Heo, lda, E, 1, 1, Ho4, lda, gA, lda)  # dpre^T [pair | third]
                copy2d(gW_ue[:, :Hne], gA[:, :Hne])
                copy2d(gW_ue[:, Hne:], gA[:, Hq:Hq + Hee])
                colsum(dpre, E, Heo, Ho4, gb_ue)
                gemm(dthird, erows, Hee, De, E, 1, 1, He4, lde, gW_ee, De)
                colsum(dthird, E, Hee, He4, gb_ee)
                if need_ge:
                    gemm(dthird, W_ee, E, De, Hee, 0, 1, He4, De, de, De4, beta=1.0)
            # dLR: over the out-edges [dfirst | dsecond] as it lies, over the in-slots with the halves swapped
            G2, G1 = dmpnn_atom_sum(g, dfs, transpose=True), dmpnn_atom_sum(g, dfs)
            if N:
                call("mvml_add_cols_f32", N, Hq, _off(G1, Hq), 2 * Hq, ptr(G2), 2 * Hq, st)
                call("mvml_add_cols_f32", N, Hq, ptr(G1), 2 * Hq, _off(G2, Hq), 2 * Hq, st)
            gx, gWlr, gblr = linear_backward(x, Wlr, G2, lm_lr, need_gx=need_gx, gx_acc=gx)
            edge_grads = (_dense(gWlr[:Hne]), _dense(gblr[:Hne]), _dense(gWlr[Hq:Hq + Hne]), _dense(gblr[Hq:Hq + Hne]),
                          gW_ee, gb_ee, gW_ue, gb_ue)
        ge = None
        if need_ge:
            ge = _dense(de[:, :De]) if ctx.slot_in or E == 0 else weave_permute_rows(g, de, De, True)
        return (gx, ge, None, None, None, gW_nn, gb_nn, gW_en, gb_en, gW_un, gb_un, *edge_grads)
