"""Record the forward norm kernels' output bits (tests/golden/norm_fwd_bits.npz).

    python tests/golden/make_norm_fwd_bits.py LIBVQA_HIP_SO OUT_NPZ        (needs the GPU)

The committed file was written by the library built from the commit before the kernels' row
arithmetic moved into csrc/norm_rows.h; tests/test_gemm_norm_gpu.py holds every later build to
those bits at D = 256, 512, 768 and 1024 (9 rows each: two blocks, the second partial).
Inputs are integer hashes scaled by powers of two, so they are the same on every host."""
import ctypes
import sys

import numpy as np

ROWS = 9


def _u(n, salt):
    i = np.arange(n, dtype=np.uint64)
    h = (i * np.uint64(2654435761) + np.uint64(salt) * np.uint64(40503)) & np.uint64(0xFFFFFFFF)
    h ^= h >> np.uint64(15)
    h = (h * np.uint64(2246822519)) & np.uint64(0xFFFFFFFF)
    h ^= h >> np.uint64(13)
    return ((h >> np.uint64(8)).astype(np.float32) / np.float32(1 << 24)) - np.float32(0.5)    # [-0.5, 0.5), exact


def inputs(D):
    x = (_u(ROWS * D, D + 1) * np.float32(8)).reshape(ROWS, D)
    x[3] *= np.float32(1 / 1024)                       # a small row
    g = np.float32(1) + _u(D, D + 2) * np.float32(0.25)
    b = _u(D, D + 3) * np.float32(0.25)
    return x, g, b


def run_norms(lib, x, g, b):
    import torch
    rows, D = x.shape
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    X, G, B = dev(x), dev(g), dev(b)
    P = lambda t: ctypes.c_void_p(t.data_ptr())
    s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    y, r = torch.empty_like(X), torch.empty(rows, device="cuda")
    ly, mu, rs = torch.empty_like(X), torch.empty(rows, device="cuda"), torch.empty(rows, device="cuda")
    assert lib.vqa_rmsnorm_fwd(P(X), P(G), P(y), None, P(r), rows, D, ctypes.c_float(1e-6), None, s) == 0
    assert lib.vqa_layernorm_fwd(P(X), P(G), P(B), P(ly), None, P(mu), P(rs), rows, D, ctypes.c_float(1e-5), s) == 0
    torch.cuda.synchronize()
    return {"rms_y32": y.cpu().numpy(), "rms_rstd": r.cpu().numpy(), "ln_y32": ly.cpu().numpy(),
            "ln_mean": mu.cpu().numpy(), "ln_rstd": rs.cpu().numpy()}


if __name__ == "__main__":
    import torch  # noqa: F401  (the library binds to the HIP runtime torch loads)
    lib = ctypes.CDLL(sys.argv[1])
    out = {}
    for D in (256, 512, 768, 1024):
        for name, a in run_norms(lib, *inputs(D)).items():
            out[f"{name}_{D}"] = a
    np.savez_compressed(sys.argv[2], **out)
    print("wrote", sys.argv[2], sorted(out))
