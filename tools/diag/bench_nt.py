"""Stand-alone timing of every NT GEMM product the C2 step launches (3 branches x 8192 rows), each alone on the GPU: the
direction net's conv1x1 forward (PReLU + stats), sconv forward (residual), dA2 / dXi of the backward and its fc layer forward
(ReLU of a ReLU input) and backward (mask by the forward output), and the same products at the restorer's channel count."""
import os, sys
root = os.environ.get("GRAFT_REPO_ROOT", os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
sys.path.insert(0, os.path.join(root, "generative-audio_amd"))
import torch
from nppc_audio import _hip as H
Z, R, Tp, Tv = 3, 8192, 256, 251
dt = torch.bfloat16
g = torch.Generator().manual_seed(0)
def mk(*shape): return (torch.randn(*shape, generator=g) * 0.1).to(dt).cuda()
def timed(fn, n=20):
    for _ in range(5): fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n): fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n * 1e3
# (name, epilogue, N, K, relu_in); epilogues 2 and 5 read a second [R][N] operand (residual / mask)
for name, epi, N, K, relu_in in (("conv1x1 fwd  (PReLU+stats) N=512 K=576", 1, 512, 576, 0), ("sconv fwd    (residual)    N=576 K=512", 2, 576, 512, 0),
                                 ("dA2 bwd      (plain)       N=512 K=576", 0, 512, 576, 0), ("dXi bwd      (residual)    N=576 K=512", 2, 576, 512, 0),
                                 ("fc fwd       (ReLU, relu_in) N=320 K=576", 3, 320, 576, 1), ("fc bwd       (mask-pos)    N=576 K=320", 5, 576, 320, 0),
                                 ("restorer conv1x1 fwd (PReLU+stats) N=512 K=320", 1, 512, 320, 0), ("restorer sconv fwd (residual) N=320 K=512", 2, 320, 512, 0),
                                 ("restorer dA2 bwd (plain)   N=512 K=320", 0, 512, 320, 0), ("restorer dXi bwd (residual) N=320 K=512", 2, 320, 512, 0)):
    A, W, res = mk(Z, R, K), mk(Z, N, K), mk(Z, R, N)
    out = torch.empty(Z, R, N, dtype=dt, device="cuda")
    slope = torch.full((Z,), 0.25, device="cuda"); stats = torch.zeros(Z, R // Tp, 2, dtype=torch.float64, device="cuda")
    has_res = epi in (2, 5)
    fn = lambda: H.call("nppc_gemm_nt", 0, epi, A, K, R * K, W, K, N * K, out, N, R * N, None, 0, res if has_res else None, N, R * N,
                        slope if epi == 1 else None, 1, stats if epi == 1 else None, (R // Tp) * 2, R, N, K, Tp, Tv, N, relu_in, Z, 1, H.stream())
    us = timed(fn)
    fl = 2.0 * Z * R * N * K
    print(f"{name}: {us:7.1f} us  {fl / us / 1e6:7.1f} TFLOP/s  operands+output {(A.numel() + W.numel() + out.numel() * (2 if has_res else 1)) * 2 / 1e6:.0f} MB", flush=True)
