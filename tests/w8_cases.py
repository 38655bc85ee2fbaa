"""Plain reference of the FP8 weight format and the shape tables of tests/test_gpu_w8.py."""
import numpy as np
import torch

SHAPES = [(16, 128), (40, 192), (2048, 1056), (1024, 2048), (512, 6144)]      # (N, K): one block; ragged rows + half block; odd block count; the o / down shapes
QUANT_SHAPES = [(N, K) for N in (16, 40) for K in (128, 192, 1056)]
MS = [1, 3, 8, 9, 16]                                                         # B-order x; crossbar half rows; its edge; full tiles

def quantize(w):
    """w [N][K] (bf16 values) -> codes u8 [N][K], exps i32 [N][nb], dequantised f64 [N][K]"""
    N, K = w.shape
    nb = (K + 127) // 128
    wp = np.zeros((N, nb * 128)); wp[:, :K] = w
    amax = np.abs(wp.reshape(N, nb, 128)).max(axis=2)
    e = np.where(amax > 0, np.ceil(np.log2(np.maximum(amax, 1e-300) / 448.0)), 0).astype(np.int32)      # smallest e with amax * 2^-e <= 448
    scale = np.repeat(np.exp2(e.astype(np.float64)), 128, axis=1)[:, :K]
    f8 = torch.from_numpy(w.astype(np.float64) / scale).to(torch.float8_e4m3fn)                           # exact quotient, RNE
    return f8.view(torch.uint8).numpy(), e, f8.to(torch.float64).numpy() * scale
