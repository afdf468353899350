"""Microbenchmark of MPNN's NNConv kernels (csrc/nnconv.hip) and of one MPNNPredictor training step
on one GPU.

On the config-3 batch with De = 10 seeded bond features, at D / H = 32/64, 64/128, 128/128:
  * mvml_nnconv_fwd, mvml_nnconv_bwd_data, mvml_nnconv_bwd_weight: ms per launch and the useful
    flops (2 H D^2 per edge and product; the data gradient is two products) as a fraction of the
    fp16 MFMA peak / 3 (the project's convention for fp32-accurate products, bench.py);
  * mvml_nnconv_bwd_weight_f16x2 (csrc/nnconv_wgrad.hip) beside the fp32 mvml_nnconv_bwd_weight in the
    same interleaved windows, and mvml_nnconv_split_z (its z image) on its own;
  * one MPNNPredictor(39, 10, D, H) training step with FlatAdam, with each weight_grad;
  * at --small-mols molecules (4,096: the per-edge matrices fit, E D^2 4 bytes), the forward against
    the materialised composition: the project's GEMM for W_e = z W2^T, then torch's bmm and
    index_add_.  That composition is timed here only; no module runs it.

Method (tools/gcn_bench.py's): device events around back-to-back launches, warm-up windows, timed
windows per variant with the variants of a comparison interleaved; median and min .. max.

    python tools/mpnn_bench.py [--mols 65536] [--sizes 32x64,64x128,128x128] [--out profiles/mpnn_bench.json]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "mvml-mpi_amd"), ROOT, os.path.join(ROOT, "tools")]
import torch  # noqa: E402

from gcn_bench import row, timed  # noqa: E402
from mvml_gat import FlatAdam, MPNNPredictor, _lib, bce_with_logits, synth  # noqa: E402
from mvml_gat import functional as Fn  # noqa: E402
from mvml_gat._lib import call, ptr  # noqa: E402

FN, DE = 39, 10
PEAK = 2500.0 / 3  # TFLOP/s: dense fp16 MFMA peak over the three products of a split-fp16 multiply


def flops_row(name, t, flops):
    r = row(name, t)
    r["tflops"] = flops / (r["ms"] * 1e9)
    r["of_peak"] = r["tflops"] / PEAK
    print(f"    {r['tflops']:8.1f} TFLOP/s useful = {100 * r['of_peak']:.1f} % of fp16 MFMA peak / 3")
    return r


def kernel_calls(g, D, H):
    """The three entries on seeded operands: {name: callable}, and the forward's operands."""
    st, L = _lib.stream_ptr(), _lib.lib()
    N, E = g.num_nodes(), g.num_edges()
    rnd = lambda *s: torch.randn(s, device="cuda")
    h, z, W2, go = rnd(N, D), rnd(E, H).relu_(), rnd(D * D, H) / (D * H) ** 0.5, rnd(N, D)
    img, sd = Fn.nnconv_image(W2, D, H), Fn.nnconv_slot_dst(g)
    out, dH, dz, dW2 = torch.empty((N, D), device="cuda"), torch.empty((N, D), device="cuda"), torch.empty_like(z), torch.empty_like(W2)
    ws = _lib.ws_ptr_size(max(L.mvml_nnconv_fwd_workspace_size(E, D), L.mvml_nnconv_bwd_data_workspace_size(E, D, H),
                              L.mvml_nnconv_bwd_weight_workspace_size(E, D, H)), "cuda")

    def fwd():
        call("mvml_nnconv_fwd", N, E, ptr(g.in_rowptr), ptr(g.in_src), ptr(h), D, D, ptr(z), H, H, ptr(img), None, ptr(out), D,
             *ws, st)

    def bwd_data():
        call("mvml_nnconv_bwd_data", N, E, ptr(g.in_src), ptr(sd), ptr(g.out_rowptr), ptr(g.out_inslot), ptr(h), D, D, ptr(z),
             H, H, ptr(img), ptr(go), D, 0, ptr(dz), H, ptr(dH), D, *ws, st)

    def bwd_weight():
        call("mvml_nnconv_bwd_weight", E, ptr(g.in_src), ptr(sd), ptr(h), D, D, ptr(z), H, H, ptr(go), D, 0, ptr(dW2), *ws, st)

    # the split-fp16 form: its z image, a result of its own (compared below) and a workspace of its own
    zimg = torch.empty(L.mvml_nnconv_z_image_bytes(E, H), dtype=torch.uint8, device="cuda")
    dW2h = torch.empty_like(W2)
    wsh = torch.empty(L.mvml_nnconv_bwd_weight_f16x2_workspace_size(E, D, H), dtype=torch.uint8, device="cuda")

    def split_z():
        call("mvml_nnconv_split_z", E, H, ptr(z), H, ptr(zimg), st)

    def bwd_weight_f16x2():
        call("mvml_nnconv_bwd_weight_f16x2", E, ptr(g.in_src), ptr(sd), ptr(h), D, D, ptr(z), H, H, ptr(go), D, 0, ptr(dW2h),
             ptr(wsh), wsh.numel(), st, ptr(zimg))
    split_z()
    return ({"fwd": fwd, "bwd_data": bwd_data, "bwd_weight": bwd_weight, "bwd_weight_f16x2": bwd_weight_f16x2,
             "split_z": split_z}, (h, z, W2, out, dW2, dW2h, zimg))


def bench_kernels(g, D, H):
    E = g.num_edges()
    calls, ops = kernel_calls(g, D, H)
    tm = timed(calls, launches=2, reps=5, warm=1)  # (the two weight gradients share every window)
    f = Fn.nnconv_flops(E, D, H)
    dW2, dW2h, zimg = ops[4:]
    res = {"fwd": flops_row(f"nnconv_fwd D={D} H={H}", tm["fwd"], f),
           "bwd_data": flops_row(f"nnconv_bwd_data D={D} H={H}", tm["bwd_data"], 2 * f),
           "bwd_weight": flops_row(f"nnconv_bwd_weight D={D} H={H} (fp32 MFMA)", tm["bwd_weight"], f),
           "bwd_weight_f16x2": flops_row(f"nnconv_bwd_weight_f16x2 D={D} H={H}", tm["bwd_weight_f16x2"], f),
           "split_z": row(f"nnconv_split_z H={H}", tm["split_z"], 4 * E * H + zimg.numel()),
           "z_image_gb": zimg.numel() / 1e9,
           "f16x2_vs_fp32_rel_diff": float((dW2h - dW2).abs().max() / dW2.abs().max())}
    a, b = res["bwd_weight"], res["bwd_weight_f16x2"]
    print(f"    fp32 / split-fp16 = {a['ms'] / b['ms']:.2f} (windows {a['min_ms']:.2f} .. {a['max_ms']:.2f} against "
          f"{b['min_ms']:.2f} .. {b['max_ms']:.2f} ms); z image {res['z_image_gb']:.2f} GB; the two results differ by "
          f"{res['f16x2_vs_fp32_rel_diff']:.1e} of max |dW2|")
    return res


def bench_materialised(g, D, H):
    """The fused forward against W_e in memory, at a batch where E D^2 4 bytes fit."""
    N, E = g.num_nodes(), g.num_edges()
    calls, (h, z, W2, out, *_) = kernel_calls(g, D, H)
    We =torch.empty((E, D * D), device="cuda")
    src, dst = g.in_src.long(), Fn.nnconv_slot_dst(g).long()

    def composed():
        Fn.gemm(z, W2, E, D * D, H, 0, 0, H, H, We, D * D)
        m = torch.bmm(h[src].unsqueeze(1), We.view(E, D, D)).squeeze(1)
        return torch.zeros((N, D), device="cuda").index_add_(0, dst, m)
    err = float((composed() - (calls["fwd"](), out)[1]).abs().max() / out.abs().max())
    tm = timed({"fused": calls["fwd"], "composed": composed}, launches=2, reps=5, warm=1)
    res = {"fused": row(f"nnconv_fwd D={D} H={H}, {g.batch_size} molecules", tm["fused"]),
           "composed": row("GEMM for W_e + bmm + index_add_", tm["composed"]), "max_rel_diff": err,
           "w_e_gb": E * D * D * 4 / 1e9}
    print(f"    fused / composed = {res['fused']['ms'] / res['composed']['ms']:.2f}; W_e {res['w_e_gb']:.2f} GB; "
          f"results differ by {err:.1e}")
    return res


def bench_step(g, D, H, x, e):
    """One training step with each weight_grad, the two models' steps interleaved window by window."""
    y = (torch.rand(g.batch_size, 11, device="cuda") < 0.5).float()

    def stepper(weight_grad):
        torch.manual_seed(0)
        model = MPNNPredictor(FN, DE, node_out_feats=D, edge_hidden_feats=H, n_tasks=11, weight_grad=weight_grad).cuda().train()
        opt = FlatAdam(model.parameters(), lr=1e-3)

        def step():
            opt.zero_grad()
            bce_with_logits(model(g, x, e), y).backward()
            opt.step()
        return step
    tm = timed({wg: stepper(wg) for wg in Fn.NNCONV_WEIGHT_GRADS}, launches=2, reps=3, warm=1)
    return {"step": row(f"MPNNPredictor D={D} H={H} step (FlatAdam)", tm["fp32"]),
            "step_split_fp16": row(f'MPNNPredictor D={D} H={H} step, weight_grad="split_fp16"', tm["split_fp16"]),
            "max_memory_gb": torch.cuda.max_memory_allocated() / 1e9}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mols", type=int, default=65536)
    ap.add_argument("--small-mols", type=int, default=4096)
    ap.add_argument("--sizes", default="32x64,64x128,128x128")
    ap.add_argument("--no-modules", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    g = synth.config3(a.mols).to_graph().to("cuda")
    gen = torch.Generator().manual_seed(0)
    x = torch.randn((g.num_nodes(), FN), generator=gen).cuda()
    e = torch.randn((g.num_edges(), DE), generator=gen).cuda()
    print(f"device: {torch.cuda.get_device_name(0)}; {g.batch_size} molecules, {g.num_nodes()} atoms, {g.num_edges()} edges")
    res = {}
    for D, H in (tuple(int(v) for v in s.split("x")) for s in a.sizes.split(",")):
        res[f"D{D}H{H}"] = bench_kernels(g, D, H)
        if not a.no_modules:
            res[f"D{D}H{H}"].update(bench_step(g, D, H, x, e))
    if a.small_mols:
        small = synth.config3(a.small_mols).to_graph().to("cuda")
        res["materialised"] = bench_materialised(small, 64, 128)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
