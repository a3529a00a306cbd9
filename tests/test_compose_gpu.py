"""nfl_compose_forward on its own: the fold of xyz_encoding_final into dir_encoding.0 / transient_encoding.0 that every weight
re-pack runs,  W' = [W[:, :256] W_fin | W[:, 256:]],  b' = b + W[:, :256] b_fin,  against torch in float64.

The kernel multiplies on the fp32 matrix cores (exact products, fp32 accumulation) and adds 256 terms per element, then
the bias: elementwise  |C - C64| <= 257 * 2^-24 * (|A| @ |B| + |addm|),  the standard bound of a 256-term fp32 sum plus one
addition.  The side columns are the caller's copy, bit for bit; without has_t the transient pair is not written."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

SENT = -12345.5
W, H = 256, 128
P_FINAL, P_DIR, P_T0 = 8, 9, 12      # NFL_P_* of include/nerf_fl_amd.h


# n_side: 4 direction frequencies (27 columns) without and with a 48-wide appearance code; n_tau 16: the layer's only shapes
@pytest.mark.parametrize("has_t", [0, 1])
@pytest.mark.parametrize("n_side", [27, 75])
def test_compose_forward_against_float64(has_t, n_side):
    import gpu_util
    from nerf_fl_amd import _lib
    n_tau = 16
    gen = torch.Generator().manual_seed(100 * n_side + has_t)
    rnd = lambda *shape: torch.randn(*shape, generator=gen).to(gpu_util.DEV)
    w_fin, b_fin = rnd(W, W) / 16, rnd(W)
    w = {P_DIR: rnd(H, W + n_side), P_T0: rnd(H, W + n_tau)}
    b = {P_DIR: rnd(H), P_T0: rnd(H)}
    fp = _lib.FieldParams()
    fp.weight[P_FINAL], fp.bias[P_FINAL] = w_fin.data_ptr(), b_fin.data_ptr()
    for L in (P_DIR, P_T0):
        fp.weight[L], fp.bias[L] = w[L].data_ptr(), b[L].data_ptr()
    # the API takes copies of the weights; the transient pair holds a sentinel where it must not be touched
    w_c = {P_DIR: w[P_DIR].clone(), P_T0: w[P_T0].clone() if has_t else torch.full_like(w[P_T0], SENT)}
    b_c = {L: torch.full_like(b[L], SENT) for L in (P_DIR, P_T0)}
    rc = _lib.lib().nfl_compose_forward(C.byref(fp), has_t, n_side, n_tau, w_c[P_DIR].data_ptr(), b_c[P_DIR].data_ptr(),
                                        w_c[P_T0].data_ptr(), b_c[P_T0].data_ptr(), torch.cuda.current_stream().cuda_stream)
    assert rc == 0
    torch.cuda.synchronize()
    eps = 257 * 2.0 ** -24
    for L in (P_DIR, P_T0) if has_t else (P_DIR,):
        a64, f64 = w[L][:, :W].double(), w_fin.double()
        err_w = (w_c[L][:, :W].double() - a64 @ f64).abs()
        bound_w = eps * (a64.abs() @ f64.abs())
        print(f"layer {L}: W' max err {err_w.max().item():.3e}, max err / bound {(err_w / bound_w).max().item():.3f}")
        assert bool((err_w <= bound_w).all())
        err_b = (b_c[L].double() - (b[L].double() + a64 @ b_fin.double())).abs()
        bound_b = eps * (a64.abs() @ b_fin.double().abs() + b[L].double().abs())
        print(f"layer {L}: b' max err {err_b.max().item():.3e}, max err / bound {(err_b / bound_b).max().item():.3f}")
        assert bool((err_b <= bound_b).all())
        assert torch.equal(w_c[L][:, W:].contiguous().view(torch.int32), w[L][:, W:].contiguous().view(torch.int32))
    if not has_t:
        assert bool((w_c[P_T0] == SENT).all()) and bool((b_c[P_T0] == SENT).all())
