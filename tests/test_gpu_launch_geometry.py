"""Every kernel of the staged, hierarchical, regulariser and shared training units past its grid cap, scan round or size switch.

The rest of the GPU suite is deep at small sizes; almost every kernel outside the fused renderers has a second regime above them
-- the second trip of a grid-stride loop, the second round of a single-workgroup scan, the unrolled part of a block sum, another
wave count per workgroup, the weight gradient's two-round grid, context offsets past 2^32 -- that the product enters and no other
test does.  The sizes come from tests/launch_geometry.py (the census that tests/test_launch_geometry_host.py holds to the
sources): the smallest count that enters each regime, with S, C and L tiny so that only the count is large.

Two yardsticks, and no bar of this file's own:
  * the existing reference at the full size -- oracle.nerf_oracle, float64 autograd, numpy host replays for the integer kernels --
    at the bar the project already asserts for that kernel at small sizes (named at each assertion);
  * period duplication, bit for bit: where a kernel's result for an item does not depend on the item's index, item cap + i is built
    as a copy of item i, and out[cap:] must equal out[:tail].  No tolerance; catches any second-trip addressing or stale-state
    error that a bar could hide under a 1 / R-scaled gradient.
The one bar size enters is the loss value: block_sum_fixed adds at most R / 256 + 9 non-negative terms in a chain (R / 256 per
thread, 6 butterfly levels, 3 adds), so the sum errs by at most (R / 256 + 9) 2^-24 relative: 1.6e-5 at R = 65 573, inside the
existing 2e-4 of check_against.  ray_terms_finish_kernel's chain is R / 1024 + 6 + 16.

Two sizes differ from what a glance at the launch expressions suggests (the census reads the kernels' loops):
  * composite_merge_kernel is one THREAD per ray, so its 16 384 workgroups take 4 194 304 rays per trip, not 65 536: its case runs
    4 194 341 rays at S + Ni = 2 + 1;
  * fetch_points_backward_kernel spends 16 lanes on a sample: 8192 workgroups take 131 072 samples per trip.
repack3_kernel is reached through a model's parameter count alone; a V3 model in the fp32 mode re-packs 1 851 232 work items, past
4096 x 256, so it has a case too.

Time on an MI355X: this file 12.5 s (46 tests, the slowest 1.4 s: Adam against torch.optim on the CPU); the parent commit's GPU suite
264.5 s (1161 tests).

RECORD (MI355X; per case the size, the regime, and the largest |a - e| / bound observed; `bits`: exact comparisons only):
  a  composite, composite_backward[_geom]   R 65 573, S 3: second trip of the ray loop     fwd 0.013, d_rgb 0.001, d_sigma 0.002,
                                                                                            d_z 0.002, d_rays_d 0.007; copies: bits
                                            R 65 573, S 16                                  fwd 0.023, d_sigma 0.317 (per ray), d_z 0.004
  a  ray_grad                               R 65 573, S 3                                   0.970 of S 2^-24 sum |terms|; copies: bits
  a  loss kernel (all terms), mse kernel    R 65 573, S 3 and 65 (two segments)             losses 4e-4 of 2e-4, d_rgb 0.008,
                                                                                            d_sigma 0.022 (S 65, per ray); ties: bits
  a  regularised / indexed loss kernels     R 65 573, S 3 and 16, dense and slot            losses 5e-4, d_rgb 0.003, d_sigma 0.003 (S 3),
                                                                                            0.051 (S 16, per ray); indexed = dense masked
                                                                                            = parent: bits
  a  composite_merge                        R 4 194 341, S + Ni 3: second trip (threads)    rgb 0.002, depth 0.010, weights 0.002 of 1e-4;
                                                                                            merge = sorted union, copies: bits
  b  mark_rays / mark_camera                R 65 573 / 257 x 256                            bits
  b  compact_rays                           R 1023, 1024, 1025, 2048, 3077, 65 573, S 5     bits (second scan round; second trip)
  c  ray_terms_finish                       R 63, 1024, 1025, 4100                          5e-4 of 2e-4; two runs: bits
  c  loss side job of adamw_step_loss       R 2047, 2048, 2049, 5000                        5e-4 of 2e-4; two runs: bits
  c  mse_grad                               n 1025                                          inside 1e-6 / 1e-7
  d  sample_along_rays                      32 769 x 64, t_rand; lindisp                    0.000 (equal to the oracle); copies: bits
  d  encode                                 n 33 296 x 63                                   0.060 of 1e-6; copies: bits
  d  project_fetch / sample_features        n 32 773 x 64                                   0.000 of 1e-5, projections 0.000; copies: bits
  d  fetch point adjoints                   n 131 109, C 64 (16-byte loads) and 66          0.001 of 2e-4; copies: bits
  d  sample_features_backward               130 x 128 x 64 map: reduce past 1 048 576       0.001 of 2e-4; two runs: bits
  d  get_rays                               1025 x 1024                                     bits
  d  occupancy_pack / dilate                2 621 440 cells / 512 x 512 x 257               bits
  d  adam_step, adamw_step_loss             n 1 048 876, two steps                          0.060 of 1e-6; copies: bits
  d  repack (nrf_model_update_device)       V3 fp32, 1 851 232 work items                   forward: bits; gradient inside 1e-5
  e  sample_pdf / sample_pdf_sorted         R 16 389, S = Ni = 8; R 9, S 1300 / 2600        0.000 of 1e-4; sorted = sort, copies: bits
  e  composite_hier_loss_backward           R 65 573, S + Ni 40 + 25: 4 262 245 samples     bits (stable sort + parent kernels)
  f  training chain V1 f32                  n 262 000, tiles32 8192, context 4 596 955 136  windows 0.028 of 2e-5; repeat, inference,
                                                                                            halving: bits
  f  training chain V1 bf16                 n 482 000, tiles32 15 064, context 4 299 110 400  windows 0.012 of 2e-5; repeat, inference: bits
  f  training chain V3 (dino 64) bf16       n 262 000, tiles32 8192, context 4 521 712 640  windows 0.013 of 2e-5; repeat, inference: bits
"""
import ctypes as C
import gc

import numpy as np
import pytest
import torch

from oracle import nerf_oracle as O
from tests import launch_geometry as G
from tests.test_gpu_multiscale_step import check_against, normals, run_loss_backward
from tests.test_gpu_ray_reg import KAPPA, compacted, oracle as reg_oracle, run_reg, skip_map
from tests.test_gpu_train_rays import NEAR, FAR, ray_batch, u01
from tests.test_gpu_training import rel_to_max
from tests.test_ray_reg_host import case

pytestmark = pytest.mark.gpu

R_RAYS = G.R_RAYS
U24 = 2.0 ** -24


@pytest.fixture(scope="module")
def N():
    import nerf_few_shot_limitations_amd as N
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from nerf_few_shot_limitations_amd import _lib
    _lib.lib()
    return N


@pytest.fixture(scope="module")
def L(N):
    from nerf_few_shot_limitations_amd import _lib as L
    return L


@pytest.fixture(autouse=True)
def _release():
    yield
    gc.collect()
    torch.cuda.empty_cache()


def dup(t, cap):
    """Rows cap ... of `t` replaced by copies of rows 0 ...: the period-duplicated input."""
    t = t.clone()
    t[cap:] = t[: t.shape[0] - cap]
    return t


def same_tail(t, cap, what=""):
    tail = t.shape[0] - cap
    assert tail > 0 and torch.equal(t[cap:], t[:tail]), f"{what}: rows past the grid's first trip differ from their copies"


def check_at(got, ref, S):
    """check_against at 1e-4 where a ray has enough samples for its form of the d_sigma bar.  check_against divides a ray's d_sigma
    error by the ray's largest |d_sigma|; at S = 3 a ray has one or two non-zero entries (the last sample's is 0: its interval is
    1e10), each a difference of terms that can cancel, and over 65 573 rays some ray's largest entry is a near-complete cancellation:
    the ORACLE in float32 against itself in float64 then shows 1.6e-2 in that form on these inputs (2e-7 relative to the tensor's
    largest entry; 2e-6 in the per-ray form at S = 65).  So at S = 3 d_sigma is held to 1e-4 of the tensor's largest entry, the form
    test_composite_backward_rgb_only asserts; prediction, losses and d_rgb keep check_against's forms and figures."""
    if S >= 16:
        return check_against(got, ref, 1e-4)
    assert (got["pred"].cpu() - ref["pred"]).abs().max() < 1e-5
    gl, rl = got["losses"].cpu().double(), ref["losses"].double()
    print("losses", gl.tolist(), rl.tolist())
    assert torch.all((gl - rl).abs() <= 2e-4 * rl.abs() + 1e-12), (gl, rl)
    e_rgb, e_sig = rel_to_max(got["d_rgb"], ref["d_rgb"]), rel_to_max(got["d_sigma"], ref["d_sigma"])
    print("d_rgb err / max", e_rgb, "d_sigma err / max", e_sig)
    assert e_rgb < 1e-4 and e_sig < 1e-4


# ---------------------------------------------------------------------------------------------
# a. the compositor family on the second trip of the ray loop
# ---------------------------------------------------------------------------------------------
def loss_inputs(R, S, seed, cap):
    """tests/test_ray_reg_host.case (a third of the densities <= 0, two equal depths per ray) without the opaque sample, one opaque
    ray (5, hence also cap + 5 in the tail), target, depth target and noise -- rows cap ... copies of rows 0 ...."""
    rgb, sig, z, d = case(R, S, seed, opaque=False)
    sig[5, S // 3] = 40.0
    tgt, tdepth, noise = u01(seed + 10, R, 3), u01(seed + 11, R) * 4 + 2, normals(seed + 12, R * S).reshape(R, S, 1)
    return [dup(t, cap) for t in (rgb, sig, z, d, tgt, tdepth, noise)]


@pytest.mark.parametrize("S,white", [(3, False), (3, True), (16, True)])
def test_composite_and_its_backwards_on_the_second_trip(N, S, white):
    """nrf_composite, nrf_composite_backward, nrf_composite_backward_geom at R = 65 573, S = 3 and 16.  Bars: the forward's 1e-5 and
    the gradients' 1e-4 of test_composite_backward_matches_autograd / test_composite_geometry_matches_autograd; d_sigma relative to
    each ray's largest entry at S = 16 as there, to the tensor's at S = 3 (check_at)."""
    from nerf_few_shot_limitations_amd import training as TR
    from tests.test_gpu_input_grad import composite_case, composite_loss
    R = G.size("composite_kernel")
    cap = G.reach(G.row("composite_kernel"))
    assert R == G.size("composite_backward_kernel") == G.size("composite_backward_geom_kernel")
    rs, z, d, g = composite_case(R, S)
    rs[5, S // 3, 3] = 40.0                                      # an opaque ray, and its copy in the tail
    rs, z, d = dup(rs, cap), dup(z, cap), dup(d, cap)
    g = {k: dup(v, cap) for k, v in g.items()}
    a = rs.cuda().requires_grad_(True)
    zc, dc = z.cuda().requires_grad_(True), d.cuda().requires_grad_(True)
    out = TR.composite(a, zc, dc, white, geom_grad=True)
    composite_loss(out, g, "cuda").backward()
    b = rs.cuda().requires_grad_(True)
    composite_loss(TR.composite(b, z.cuda(), d.cuda(), white), g, "cuda").backward()
    assert torch.equal(a.grad, b.grad)                          # the geometry kernel's d_rgb / d_sigma are the plain kernel's bits
    ro, zo, do = (t.double().requires_grad_(True) for t in (rs, z, d))
    ref = O.volume_render(ro[..., :3], ro[..., 3:4], zo, do, white)
    composite_loss(ref, {k: v.double() for k, v in g.items()}).backward()
    e_fwd = float((out[0].detach().cpu() - ref[0].detach()).abs().max())
    e_rgb = rel_to_max(b.grad[..., :3], ro.grad[..., :3])
    ds, es = b.grad[..., 3].cpu().double(), ro.grad[..., 3]
    e_sig = float(((ds - es).abs() / es.abs().amax(dim=1, keepdim=True).clamp_min(1e-20)).max()) if S >= 16 else rel_to_max(ds, es)
    e_z, e_d = rel_to_max(zc.grad, zo.grad), rel_to_max(dc.grad, do.grad)
    print(f"\nRECORD a composite R {R} S {S} white {white}: fwd {e_fwd / 1e-5:.3f} d_rgb {e_rgb / 1e-4:.3f} d_sigma {e_sig / 1e-4:.3f} "
          f"d_z {e_z / 1e-4:.3f} d_rays_d {e_d / 1e-4:.3f} of their bars")
    assert e_fwd < 1e-5 and e_rgb < 1e-4 and e_sig < 1e-4 and e_z <= 1e-4 and e_d <= 1e-4
    assert torch.isfinite(zc.grad).all() and torch.isfinite(dc.grad).all()
    for name, t in (("rgb", out[0]), ("depth", out[1]), ("weights", out[2]), ("d_rows", a.grad), ("d_z", zc.grad), ("d_rays_d", dc.grad)):
        same_tail(t.detach(), cap, name)


def test_ray_grad_on_the_second_trip(L):
    """nrf_ray_grad at R = 65 573, S = 3: test_ray_grad_matches_its_definition's bound, S 2^-24 of the terms' magnitudes."""
    R, S = G.size("ray_grad_kernel"), 3
    cap = G.reach(G.row("ray_grad_kernel"))
    dp, dd = dup(u01(71, R, S, 3) - 0.5, cap).reshape(R * S, 3), dup(u01(72, R, S, 3) - 0.5, cap).reshape(R * S, 3)
    z, d = dup(2 + 4 * u01(73, R, S), cap), dup(u01(74, R, 3) - 0.5, cap)
    dz_in, dd_in = dup(u01(75, R, S) - 0.5, cap), dup(u01(76, R, 3) - 0.5, cap)

    def run():
        t = [x.cuda().contiguous() for x in (dp, dd, z, d, dz_in, dd_in)]
        o = [torch.full((R, 3), float("nan"), device="cuda"), torch.full((R, 3), float("nan"), device="cuda"), torch.full((R, S), float("nan"), device="cuda")]
        L.check(L.lib().nrf_ray_grad(*[L.ptr(x) for x in t], R, S, *[L.ptr(x) for x in o], L.stream_ptr()))
        torch.cuda.synchronize()
        return [x.cpu() for x in o]
    a, b = run(), run()
    P, Dd, Z, D = dp.double().reshape(R, S, 3), dd.double().reshape(R, S, 3), z.double(), d.double()
    want_d = (Z[..., None] * P + Dd).sum(1) + dd_in.double()
    mag_d = ((Z[..., None] * P).abs() + Dd.abs()).sum(1) + dd_in.double().abs()
    want_z = (D[:, None, :] * P).sum(-1) + dz_in.double()
    mag_z = (D[:, None, :] * P).abs().sum(-1) + dz_in.double().abs()
    worst = 0.0
    for got, again, want, mag in ((a[0], b[0], P.sum(1), P.abs().sum(1)), (a[1], b[1], want_d, mag_d), (a[2], b[2], want_z, mag_z)):
        assert torch.equal(got, again)
        worst = max(worst, float(((got.double() - want).abs() / (S * U24 * mag + 1e-300)).max()))
        same_tail(got, cap, "ray_grad")
    print(f"\nRECORD a ray_grad R {R} S {S}: {worst:.3f} of S 2^-24 sum|terms|")
    assert worst <= 1.0


@pytest.mark.parametrize("S", [3, 65])
def test_loss_kernels_on_the_second_trip(L, S):
    """nrf_composite_mse_backward (with the clearing side job) and nrf_composite_loss_backward (all terms, depth target, noise
    tensor, white background) at R = 65 573; S = 65 walks the two-segment path on the second trip too.  check_against's bars at
    1e-4 (check_at: its d_sigma form at S = 3), the loss within 2e-4 (the derivation in the module docstring)."""
    R = G.size("composite_loss_backward_kernel<true>")
    cap = G.reach(G.row("composite_loss_backward_kernel<true>"))
    assert R == G.size("composite_loss_backward_kernel<false>") and (R / 256 + 9) * U24 < 2e-4
    rgb, sig, z, d, tgt, tdepth, noise = loss_inputs(R, S, 300 + S, cap)
    w, std = (0.7, 0.3, 0.5), 0.4
    got = run_loss_backward(L, rgb, sig, z, d, tgt, True, w, tdepth, std, noise, zero_n=100003)
    ref = reg_oracle(rgb, sig, z, d, tgt, True, w, tdepth, std, noise, 0.0, 0.0, 0)
    ref["losses"] = ref["losses"][:4]
    print(f"\nRECORD a loss kernel R {R} S {S}:")
    check_at(got, ref, S)
    assert torch.all(got["zero"] == 0)
    eff = sig[..., 0] + noise[..., 0] * std
    assert (eff[cap:] <= 0).any() and torch.all(got["d_sigma"].cpu()[eff <= 0] == 0)
    for k in ("pred", "d_rgb", "d_sigma"):
        same_tail(got[k], cap, k)
    same_tail(got["terms"].T.contiguous(), cap, "terms")
    again = run_loss_backward(L, rgb, sig, z, d, tgt, True, w, tdepth, std, noise, zero_n=100003)
    for k in ("pred", "d_rgb", "d_sigma", "terms", "losses"):
        assert torch.equal(again[k], got[k]), k
    # the MSE kernel: the loss kernel with every option off, bit for bit (test_all_options_off_is_the_mse_kernel_bit_for_bit), at this R
    off = run_loss_backward(L, rgb, sig, z, d, tgt, True, (0.7, 0.0, 0.0), with_losses=False)
    c, s_ = rgb.contiguous().cuda(), sig.reshape(R, S).contiguous().cuda()
    pred, d_rgb, d_sig, rl = torch.empty(R, 3, device="cuda"), torch.empty(R, S, 3, device="cuda"), torch.empty(R, S, device="cuda"), torch.empty(R, device="cuda")
    zc, dc, tc, junk = z.cuda(), d.cuda(), tgt.cuda(), torch.ones(100003, device="cuda")
    L.check(L.lib().nrf_composite_mse_backward(L.ptr(c), 3, L.ptr(s_), 1, L.ptr(zc), L.ptr(dc), R, S, 1, L.ptr(tc), 0.7, L.ptr(pred), L.ptr(d_rgb), 3,
                                               L.ptr(d_sig), 1, L.ptr(rl), L.ptr(junk), junk.numel(), L.stream_ptr()))
    torch.cuda.synchronize()
    assert torch.equal(off["pred"], pred) and torch.equal(off["d_rgb"], d_rgb) and torch.equal(off["d_sigma"], d_sig) and torch.equal(off["terms"][0], rl)
    assert torch.all(junk == 0)
    for k, t in (("pred", pred), ("d_rgb", d_rgb), ("d_sigma", d_sig), ("ray_loss", rl)):
        same_tail(t, cap, "mse " + k)


@pytest.mark.parametrize("S", [3, 16])
def test_indexed_and_regularised_loss_kernels_on_the_second_trip(L, S):
    """nrf_composite_reg_loss_backward dense and with `slot`, both terms on, and nrf_composite_loss_backward_indexed, at R = 65 573,
    S = 3 and 16: the dense entry against float64 autograd (check_at, 1e-4), the indexed entry against the dense one on masked rows bit
    for bit (test_indexed_entry_is_the_dense_entry_on_masked_rows_and_runs_repeat), the indexed parent against the regularised entry
    with the terms off bit for bit (test_options_off_are_the_parents_bits)."""
    R, k = G.size("reg_loss_backward_kernel<true>"), 2
    cap = G.reach(G.row("reg_loss_backward_kernel<true>"))
    assert R == G.size("reg_loss_backward_kernel<false>") == G.size("indexed_loss_backward_kernel")
    rgb, sig, z, d, tgt, tdepth, noise = loss_inputs(R, S, 400 + S, cap)
    w, std = (0.7, 0.3, 0.5), 0.4
    reg = L.ray_reg(0.6, KAPPA, 0.8, k)
    dense_plain = run_reg(L, rgb, sig, z, d, tgt, True, w, tdepth, std, noise, reg)
    ref = reg_oracle(rgb, sig, z, d, tgt, True, w, tdepth, std, noise, 0.6, 0.8, k)
    print(f"\nRECORD a regularised loss kernel R {R} S {S}:")
    check_at(dense_plain, ref, S)
    assert dense_plain["losses"][4].item() > 0 and dense_plain["losses"][5].item() > 0
    for key in ("pred", "d_rgb", "d_sigma"):
        same_tail(dense_plain[key], cap, key)
    same_tail(dense_plain["terms"].T.contiguous(), cap, "terms")
    # indexed against dense on masked rows
    keep = dup(skip_map(R, S, 85, k), cap)
    frac = 1.0 - keep.float().mean().item()
    assert 0.3 < frac < 0.6, frac
    rc, sc, slot = compacted(rgb, sig, keep)
    idx = run_reg(L, rc, sc, z, d, tgt, True, w, tdepth, std, noise, reg, slot=slot)
    rgb_m = torch.where(keep[..., None], rgb, torch.zeros_like(rgb))
    sig_m = torch.where(keep[..., None], sig, torch.full_like(sig, float("-inf")))
    dense = run_reg(L, rgb_m, sig_m, z, d, tgt, True, w, tdepth, std, noise, reg)
    assert torch.equal(idx["pred"], dense["pred"]) and torch.equal(idx["terms"], dense["terms"]) and torch.equal(idx["losses"], dense["losses"])
    assert torch.isfinite(idx["terms"]).all() and torch.isfinite(idx["losses"]).all()
    flat = keep.reshape(-1).cuda()
    assert torch.equal(idx["d_rgb"], dense["d_rgb"].reshape(-1, 3)[flat]) and torch.equal(idx["d_sigma"], dense["d_sigma"].reshape(-1)[flat])
    assert torch.all(dense["d_sigma"].reshape(-1)[~flat] == 0)
    assert torch.all(idx["terms"][3:, 1] == 0) and torch.all(idx["terms"][3:, cap + 1] == 0)      # the ray that keeps no sample, and its copy
    for key in ("pred", "d_rgb", "d_sigma"):
        same_tail(dense[key], cap, "masked " + key)
    again = run_reg(L, rc, sc, z, d, tgt, True, w, tdepth, std, noise, reg, slot=slot)
    for key in ("pred", "d_rgb", "d_sigma", "terms", "losses"):
        assert torch.equal(again[key], idx[key]), key
    # the indexed parent is the regularised entry with the terms off
    lib, st = L.lib(), L.stream_ptr()
    M = rc.shape[0]
    c, s_, zc, dc, tc, td, nz, sl = (t.contiguous().cuda() for t in (rc, sc, z, d, tgt, tdepth, noise.reshape(R, S), slot))
    pred, d_rgb, d_sig, terms = torch.empty(R, 3, device="cuda"), torch.full((M, 3), 7.0, device="cuda"), torch.full((M,), 7.0, device="cuda"), torch.empty(3, R, device="cuda")
    lo = L.loss_opts(w[0], w[2], w[1], L.ptr(td), std, L.ptr(nz), 0)
    L.check(lib.nrf_composite_loss_backward_indexed(L.ptr(c), 3, L.ptr(s_), 1, L.ptr(zc), L.ptr(dc), R, S, 1, L.ptr(tc), C.byref(lo), sl.data_ptr(),
                                                    L.ptr(pred), L.ptr(d_rgb), 3, L.ptr(d_sig), 1, L.ptr(terms), None, 0, st))
    torch.cuda.synchronize()
    off = run_reg(L, rc, sc, z, d, tgt, True, w, tdepth, std, noise, reg=L.ray_reg(), slot=slot, with_losses=False)
    assert torch.equal(off["pred"], pred) and torch.equal(off["d_rgb"], d_rgb) and torch.equal(off["d_sigma"], d_sig)
    assert torch.equal(off["terms"][:3], terms)
    same_tail(pred, cap, "indexed pred")
    same_tail(terms.T.contiguous(), cap, "indexed terms")


# ---------------------------------------------------------------------------------------------
# b. occupancy marks and compaction
# ---------------------------------------------------------------------------------------------
def test_marks_on_the_second_trip(N, L):
    """nrf_occupancy_mark_rays at R = 65 573 and nrf_occupancy_mark_camera on a 257 x 256 frame against the numpy replay of
    tests/test_gpu_occupancy_mark.py: equal bits."""
    from tests.test_gpu_occupancy import T
    from tests.test_gpu_occupancy_mark import LEGO, LO1, HI1, RES1, empty_grid, mark_raw, replay, synthetic_weights, words_of
    H, W, S = 257, 256, 5
    assert H * W == G.SHAPED["occupancy_mark_kernel<true>"] > G.reach(G.row("occupancy_mark_kernel<true>"))
    R = G.size("occupancy_mark_kernel<false>")
    ro, rd = N.get_rays(H, W, O.focal_for(W), T(LEGO))
    ro, rd = ro.reshape(-1, 3).contiguous(), rd.reshape(-1, 3).contiguous()
    pts, z = N.sample_points_along_rays(ro, rd, NEAR, FAR, S, perturb=False)
    w = synthetic_weights(H * W, S, 1234)
    wt = torch.from_numpy(w).cuda()
    grid = empty_grid(N, RES1, LO1, HI1)
    tau, eps = 2.0 ** -6, 2.0 ** -7
    pts = pts.cpu().numpy()
    # the ray entry: the frame's rays rolled so that the rays past the first trip are 37 pixels of the middle row; they alone carry
    # weight on sample 2 (near the box's centre), so the second trip marks cells that no earlier ray marks
    cap = G.reach(G.row("occupancy_mark_kernel<false>"))
    order = (torch.arange(H * W) - (cap - (128 * W + 110))) % (H * W)
    order = order[:R]
    wr = w[order.numpy()].copy()
    wr[:cap, 2] = 0
    wr[cap:] = 0
    wr[cap:, 2] = 0.5
    pr = pts[order.numpy()]
    od = order.cuda()
    want_hit, want_seen = replay(grid, pr, wr, tau, eps)
    head_hit, _ = replay(grid, pr[:cap], wr[:cap], tau, eps)
    assert want_hit.sum() > 100 and want_seen.sum() > want_hit.sum() and (want_hit & ~head_hit).any()
    hit, seen = mark_raw(N, grid, ro[od].contiguous(), rd[od].contiguous(), z[od].contiguous(), torch.from_numpy(wr).cuda(), tau, eps)
    torch.cuda.synchronize()
    assert torch.equal(hit.cpu(), words_of(N, grid, want_hit)) and torch.equal(seen.cpu(), words_of(N, grid, want_seen))
    # the camera entry over the whole frame
    want_hit, want_seen = replay(grid, pts, w, tau, eps)
    got_hit, got_seen = torch.zeros_like(grid.bits), torch.zeros_like(grid.bits)
    c2w = (C.c_float * 12)(*LEGO[:3, :4].reshape(-1).tolist())
    L.check(L.lib().nrf_occupancy_mark_camera(H, W, O.focal_for(W), c2w, 0, H * W, S, L.ptr(z), L.ptr(wt), (C.c_int32 * 3)(*grid.res),
                                              (C.c_float * 3)(*grid.lo), (C.c_float * 3)(*grid.scale), tau, eps, got_hit.data_ptr(),
                                              got_seen.data_ptr(), L.stream_ptr()))
    torch.cuda.synchronize()
    assert torch.equal(got_hit.cpu(), words_of(N, grid, want_hit)) and torch.equal(got_seen.cpu(), words_of(N, grid, want_seen))


SCAN = G.reach(G.row("occupancy_compact_scan_kernel"))


@pytest.mark.parametrize("R", [SCAN - 1, SCAN, SCAN + 1, 2 * SCAN, 3 * SCAN + 5, G.size("occupancy_compact_count_kernel")])
def test_compaction_past_a_scan_round_and_past_the_grid(N, R):
    """nrf_occupancy_compact_rays around the scan kernel's 1024-ray round (carry, several rounds, a ragged last one) and on the second
    trip of the count / write kernels, S = 5, under a grid that keeps about half the samples, with one ray that keeps none: count,
    index, slot, positions and directions against the numpy replay (exclusive cumulative sum of the per-ray keep counts), exactly."""
    from tests.test_gpu_train_occupancy import check_compaction, compact, grid_of
    assert SCAN == 1024 and G.size("occupancy_compact_count_kernel") == G.size("occupancy_compact_write_kernel")
    S = 5
    o, d = ray_batch(R, seed=520)
    o = o.clone()
    o[3] = 40.0                                                 # every sample outside the box, and outside = 1: nothing kept
    grid = grid_of("random", outside=1, box=(-12.0, 12.0), seed=521)
    _, z = N.sample_points_along_rays(o, d, NEAR, FAR, S, perturb=False)
    c = compact(grid, S, o, d)
    keep = check_compaction(c, grid, o, d, z, ("scan", R))
    assert 0.3 < keep.mean() < 0.7 and not keep[3].any()        # about half (the grid has 2048 cells: the rays' share varies)
    # the replay's offsets, spelt out: the exclusive cumulative sum of the rays' keep counts
    counts = keep.sum(1)
    first = np.concatenate([[0], np.cumsum(counts)[:-1]])
    slot = c["slot"].cpu().numpy().reshape(R, S)
    has = counts > 0
    assert np.array_equal(np.where(keep, slot, np.iinfo(np.int32).max).min(1)[has], first[has]) and c["M"] == int(counts.sum())


# ---------------------------------------------------------------------------------------------
# c. single-workgroup reductions
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R", [63, SCAN, SCAN + 1, 4100])
def test_ray_terms_finish_past_its_stride(L, R):
    """nrf_ray_terms_finish: one workgroup, stride 1024 -- whole waves of zeros at R = 63, the second trip from 1025.  The float64
    sums at the existing 2e-4 relative bar (check_against's loss bar); two runs give equal bits."""
    assert G.reach(G.row("ray_terms_finish_kernel")) == SCAN
    terms = torch.cat([torch.full((3, R), float("nan")), u01(601, 2, R) * torch.tensor([[0.3], [2.0]])]).cuda().contiguous()
    l4 = torch.tensor([0.37, 0.2, 0.1, 0.05], device="cuda")
    dw, ow = 0.6, 0.8
    reg = L.ray_reg(dw, KAPPA, ow, 4)
    outs = []
    for _ in range(2):
        l6 = torch.full((6,), float("nan"), device="cuda")
        L.check(L.lib().nrf_ray_terms_finish(L.ptr(terms), R, C.byref(reg), L.ptr(l4), L.ptr(l6), L.stream_ptr()))
        torch.cuda.synchronize()
        outs.append(l6.cpu())
    assert torch.equal(outs[0], outs[1])
    md, mo = terms[3].double().mean().item(), terms[4].double().mean().item()
    l4d = l4.cpu().double()
    want = torch.stack([l4d[0] + dw * md + ow * mo, l4d[1], l4d[2], l4d[3], torch.tensor(md, dtype=torch.float64), torch.tensor(mo, dtype=torch.float64)])
    err = ((outs[0].double() - want).abs() / (2e-4 * want.abs() + 1e-12)).max().item()
    print(f"\nRECORD c ray_terms_finish R {R}: {err:.4f} of the 2e-4 bar")
    assert torch.equal(outs[0][1:4], l4[1:4].cpu()) and err <= 1.0


@pytest.mark.parametrize("R", [2047, 2048, 2049, 5000])
def test_loss_side_job_past_the_unrolled_block_sum(L, R):
    """The loss side job of nrf_adamw_step_loss, all four terms, around the size from which every thread runs block_sum_fixed's
    8 x 256 unrolled loop (2048; thread 0 enters it from 1793) and with a ragged rest behind it: float64 sums at the existing 2e-4 relative bar; two runs give equal bits."""
    S, w = 7, (0.7, 0.3, 0.5)
    terms = (u01(611, 3, R) * torch.tensor([[1.0], [3.0], [0.5]])).cuda().contiguous()
    outs = []
    for _ in range(2):
        p, g, m, v = (torch.zeros(4, device="cuda") for _ in range(4))
        losses = torch.full((4,), float("nan"), device="cuda")
        L.check(L.lib().nrf_adamw_step_loss(L.ptr(p), L.ptr(g), L.ptr(m), L.ptr(v), 4, 1e-3, 0.9, 0.999, 1e-8, 0.0, 1, 0, 0.0, None, None, L.ptr(terms),
                                            R, S, w[0], w[1], w[2], L.ptr(losses), L.stream_ptr()))
        torch.cuda.synchronize()
        outs.append(losses.cpu())
    assert torch.equal(outs[0], outs[1])
    t = terms.double().cpu()
    rgb, reg, depth = t[0].sum() / (3 * R), t[1].sum() / (R * S), t[2].sum() / R
    want = torch.stack([w[0] * rgb + w[1] * depth + w[2] * reg, rgb, depth, reg])
    err = ((outs[0].double() - want).abs() / (2e-4 * want.abs() + 1e-12)).max().item()
    print(f"\nRECORD c loss side job R {R}: {err:.4f} of the 2e-4 bar")
    assert err <= 1.0


def test_mse_grad_past_its_stride(L):
    """nrf_mse_grad just past one round of its single workgroup: test_mse_grad_kernel_matches_torch's bars."""
    n = G.size("mse_grad_kernel")
    pred, tgt = u01(121, n).cuda(), u01(122, n).cuda()
    g, loss = torch.empty(n, device="cuda"), torch.empty((), device="cuda")
    L.check(L.lib().nrf_mse_grad(L.ptr(pred), L.ptr(tgt), n, 0.7, L.ptr(g), L.ptr(loss), L.stream_ptr()))
    torch.cuda.synchronize()
    ref = 0.7 * ((pred.double() - tgt.double()) ** 2).mean()
    assert abs(loss.item() - ref.item()) < 1e-6 * max(1.0, abs(ref.item()))
    assert (g.double() - 0.7 * 2 * (pred.double() - tgt.double()) / n).abs().max() < 1e-7


# ---------------------------------------------------------------------------------------------
# d. element-per-thread kernels just past cap x items, ragged
# ---------------------------------------------------------------------------------------------
def test_sample_along_rays_on_the_second_trip(N):
    """nrf_sample_along_rays at 32 769 rays x 64 with t_rand given, and once with lindisp: test_samples_golden's bars against the
    oracle (z 5e-7 / points 2e-6; lindisp 1e-6 / 3e-6), and ray 32 768 -- the first item of the second trip -- a copy of ray 0."""
    from tests.test_gpu_parity import maxdiff
    S = 64
    R, cap = G.SHAPED["sample_kernel"] // S, G.reach(G.row("sample_kernel")) // S
    assert R * S > G.reach(G.row("sample_kernel")) and R == cap + 1
    o, d = ray_batch(R, seed=700)
    o, d, tr = dup(o, cap), dup(d, cap), dup(u01(703, R, S), cap)
    pts, z = N.sample_points_along_rays(o, d, NEAR, FAR, S, t_rand=tr.cuda())
    opts, oz = O.sample_points_along_rays(o.cpu(), d.cpu(), NEAR, FAR, S, t_rand=tr)
    e = (maxdiff(z, oz) / 5e-7, maxdiff(pts, opts) / 2e-6)
    same_tail(z, cap, "z"), same_tail(pts, cap, "pts")
    pl, zl = N.sample_points_along_rays(o, d, NEAR, FAR, S, perturb=False, lindisp=True)
    opl, ozl = O.sample_points_along_rays(o.cpu(), d.cpu(), NEAR, FAR, S, lindisp=True)
    el = (maxdiff(zl, ozl) / 1e-6, maxdiff(pl, opl) / 3e-6)
    same_tail(zl, cap, "z lindisp"), same_tail(pl, cap, "pts lindisp")
    print(f"\nRECORD d sample {R} x {S}: z {e[0]:.3f} pts {e[1]:.3f} lindisp z {el[0]:.3f} pts {el[1]:.3f} of their bars")
    assert max(e) <= 1.0 and max(el) <= 1.0


def test_encode_on_the_second_trip(N):
    """nrf_encode with n x 63 just above 2 097 152 outputs: test_encoding_golden's 1e-6 against the oracle; the second trip starts
    inside row 33 288, and that row and the ones behind it are copies of rows 0 ...."""
    from tests.test_gpu_parity import maxdiff
    reach = G.reach(G.row("encode_kernel"))
    n = G.SHAPED["encode_kernel"] // 63
    first = reach // 63                                         # the row the second trip starts in
    assert n * 63 == G.SHAPED["encode_kernel"] > reach and 0 < n - first < 64
    x = dup(u01(711, n, 3) * 2 - 1, first)
    e = N.PositionalEncoding(10)(x.cuda())
    err = maxdiff(e, O.positional_encoding(x, 10))
    print(f"\nRECORD d encode n {n}: {err / 1e-6:.3f} of 1e-6")
    assert e.shape == (n, 63) and err <= 1e-6
    same_tail(e, first, "encoding")


def test_fetches_on_the_second_trip(L):
    """nrf_project_fetch and nrf_sample_features with n x 64 just above 2 097 152 features, some taps off the map: features against
    the oracle's fetch at the kernel's own projections within 1e-5, the projections within 2e-4 (1 + |xy|) (test_project_fetch_golden's
    bars); rows 32 768 ... copies of rows 0 ...."""
    from tests.test_gpu_dino_grad import FOCAL, POSE, dino_struct, points_2d
    from tests.test_gpu_parity import maxdiff
    Cc, Hp, Wp = 64, 9, 9
    n, cap = G.SHAPED["project_fetch_kernel"] // Cc, G.reach(G.row("project_fetch_kernel", cap_text="grid_for(n * C, kBlock, 8192)")) // Cc
    assert n * Cc > cap * Cc and n - cap == 5
    fmap = (u01(721, 1, Hp, Wp, Cc) * 2 - 1).cuda()
    xy = dup(points_2d(n, 722), cap).cuda()
    f2 = torch.empty((n, Cc), device="cuda")
    L.check(L.lib().nrf_sample_features(L.ptr(fmap), Hp, Wp, Cc, L.ptr(xy), n, L.ptr(f2), L.stream_ptr()))
    p = u01(723, n, 3) * 4 - 2                                   # 1 .. 5 in front of POSE's camera; a tenth far off axis: off the map
    p[n // 10: n // 5, 0] *= 6.0
    p = dup(p, cap).cuda()
    f3, xy3 = torch.empty((n, Cc), device="cuda"), torch.empty((n, 2), device="cuda")
    d = dino_struct(L, Hp, Wp, Cc, fmap)
    L.check(L.lib().nrf_project_fetch(C.byref(d), L.ptr(p), n, L.ptr(f3), L.ptr(xy3), L.stream_ptr()))
    torch.cuda.synchronize()
    e2 = maxdiff(f2, O.sample_features_at_points(fmap.cpu(), xy.cpu()))
    ref_xy = O.project_points_to_image(p.cpu(), torch.tensor(POSE), FOCAL, 128, 128)[0].double().numpy()
    exy = float(np.max(np.abs(xy3.cpu().numpy() - ref_xy) / (2e-4 * (1 + np.abs(ref_xy)))))
    e3 = maxdiff(f3, O.sample_features_at_points(fmap.cpu(), xy3.cpu()))
    off2, off3 = float((f2.abs().sum(-1) == 0).float().mean()), float((f3.abs().sum(-1) == 0).float().mean())
    print(f"\nRECORD d fetch n {n}: 2-d {e2 / 1e-5:.3f}, world {e3 / 1e-5:.3f} of 1e-5, projections {exy:.3f} of their bar; off the map {off2:.2f} / {off3:.2f}")
    assert 0.01 < off2 < 0.9 and 0.01 < off3 < 0.9
    assert e2 <= 1e-5 and e3 <= 1e-5 and exy <= 1.0
    for name, t in (("sample_features", f2), ("project_fetch", f3), ("xy", xy3)):
        same_tail(t, cap, name)


@pytest.mark.parametrize("Cc", [64, 66])
def test_fetch_point_adjoints_on_the_second_trip(L, Cc):
    """nrf_project_fetch_backward_points and nrf_sample_features_backward_points at 8192 x 16 + 37 samples (16 lanes per sample, 16
    samples per workgroup), the 16-byte-load branch (C = 64) and the scalar one (C = 66): test_fetch_adjoint_matches_autograd's bar,
    2e-4 of the result's largest element over the samples off the texel edges; rows past the first trip copies of rows 0 ...."""
    from tests.test_gpu_point_grad import fetch_points_T, fetch_reference, views
    kernel = "fetch_points_backward_kernel<true>" if Cc % 4 == 0 else "fetch_points_backward_kernel<false>"
    n, cap = G.size(kernel), G.reach(G.row(kernel))
    r, v = fetch_reference((9, 9, Cc), cap, "orbit"), views()["orbit"]
    ext = lambda t: torch.cat([t, t[: n - cap]])
    fmap, pts, g, xy = r["fmap"].cuda(), ext(r["pts"]).cuda(), ext(r["g"]).cuda(), ext(r["xy"]).cuda().contiguous()
    keep, on = ext(r["keep"]), ext(r["on"])
    d_pts, d_xy = fetch_points_T(L, fmap, v, pts, g).cpu(), fetch_points_T(L, fmap, v, xy, g).cpu()
    assert float(keep.float().mean()) >= 0.9 and torch.isfinite(d_pts).all() and torch.isfinite(d_xy).all()
    far = ~on & keep
    assert not d_pts[far].any() and not d_xy[far].any()
    for name, got, want in (("d_points", d_pts, ext(r["d_pts"])), ("d_xy", d_xy, ext(r["d_xy"]))):
        e = rel_to_max(got[keep], want[keep])
        print(f"\nRECORD d fetch adjoint C {Cc} n {n} {name}: {e / 2e-4:.3f} of 2e-4")
        assert e <= 2e-4
        same_tail(got, cap, name)


def test_map_gradient_reduce_on_the_second_trip(L):
    """nrf_sample_features_backward on a 130 x 128 x 64 map: fetch_backward_reduce_kernel past 1 048 576 elements (texel rows 128 and
    129), against autograd through the oracle's tap-by-tap fetch at test_fetch_backward_is_the_adjoint_of_the_fetch's 2e-4 of the maximum."""
    from tests.test_gpu_dino_grad import fetch_T, points_2d
    Hp, Wp, Cc = 130, 128, 64
    assert Hp * Wp * Cc == G.SHAPED["fetch_backward_reduce_kernel"] > G.reach(G.row("fetch_backward_reduce_kernel"))
    first_row = G.reach(G.row("fetch_backward_reduce_kernel")) // (Wp * Cc)
    n = 5037
    xy = points_2d(n, 731)
    xy[1000:1300, 1] = 0.975 + 0.03 * u01(732, 300)             # taps in the last texel rows, some past the border
    g = u01(733, n, Cc) - 0.5
    d_map = fetch_T(L, (1, Hp, Wp, Cc), xy.cuda(), g.cuda())
    again = fetch_T(L, (1, Hp, Wp, Cc), xy.cuda(), g.cuda())
    torch.cuda.synchronize()
    mm = torch.zeros((1, Hp, Wp, Cc), requires_grad=True)
    (O.sample_features_at_points(mm, xy) * g).sum().backward()
    err = rel_to_max(d_map, mm.grad)
    print(f"\nRECORD d map gradient {Hp} x {Wp} x {Cc}: {err / 2e-4:.3f} of 2e-4")
    assert torch.equal(d_map, again) and err <= 2e-4
    assert mm.grad[0, first_row:].abs().max() > 0.1 * mm.grad.abs().max()        # the second trip's elements carry gradient
    assert rel_to_max(d_map[0, first_row:], mm.grad[0, first_row:]) <= 2e-4


def test_get_rays_on_the_second_trip(N):
    """nrf_get_rays on a 1025 x 1024 frame against the oracle, bit for bit (test_get_rays_full_frame_matches_oracle_bitwise)."""
    from tests.test_gpu_parity import T
    H, W = 1025, 1024
    assert H * W == G.SHAPED["get_rays_kernel"] > G.reach(G.row("get_rays_kernel"))
    c2w = T(O.LEGO_LIKE_C2W)
    ro, rd = N.get_rays(H, W, O.focal_for(W), c2w)
    oo, od = O.get_rays(H, W, O.focal_for(W), c2w)
    assert torch.equal(rd.cpu(), od) and torch.equal(ro.cpu(), oo.contiguous())


def test_pack_on_the_second_trip(L):
    """nrf_occupancy_pack on 160 x 128 x 128 cells, two densities per cell, NaNs among them: the words of a numpy replay, and the
    cells past the first trip copies of cells 0 ...."""
    n_cells, k, thr = 160 * 128 * 128, 2, 0.25
    cap = G.reach(G.row("occupancy_pack_kernel"))
    assert n_cells > cap and cap % 32 == 0
    dens = dup(u01(741, n_cells, k) * 0.3, cap)                 # a cell is occupied when one of its two values exceeds 0.25: about 30 %
    dens[::1009, 1] = float("nan")
    dens = dup(dens, cap)
    bits = torch.full((n_cells // 32,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    dd = dens.cuda().contiguous()
    L.check(L.lib().nrf_occupancy_pack(L.ptr(dd), n_cells, k, thr, bits.data_ptr(), L.stream_ptr()))
    torch.cuda.synchronize()
    occ = (~(dens.numpy() <= np.float32(thr))).any(-1)
    want = np.packbits(occ.reshape(-1, 32), axis=1, bitorder="little").view(np.uint32).reshape(-1)
    assert 0.2 < occ.mean() < 0.4 and np.array_equal(bits.cpu().numpy().view(np.uint32), want)
    same_tail(bits, cap // 32, "bits")
    # a count that ends in the middle of a wave's 64 cells (the entry takes multiples of 32): its upper word is not stored
    m = G.size("occupancy_pack_kernel")
    assert m % 64 == 32
    part = torch.full(((m + 31) // 32 + 1,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    L.check(L.lib().nrf_occupancy_pack(L.ptr(dd), m, k, thr, part.data_ptr(), L.stream_ptr()))
    torch.cuda.synchronize()
    pad = np.zeros((m + 31) // 32 * 32, dtype=bool)
    pad[:m] = occ[:m]
    got = part.cpu().numpy().view(np.uint32)
    assert np.array_equal(got[:(m + 31) // 32], np.packbits(pad.reshape(-1, 32), axis=1, bitorder="little").view(np.uint32).reshape(-1))
    assert got[-1] == 0x5A5A5A5A


def test_dilate_on_the_second_trip(N):
    """nrf_occupancy_dilate on a 512 x 512 x 257 grid, 2 105 344 words: the last z slab is the second trip.  Against the numpy
    dilation of tests/test_gpu_occupancy.py, exactly."""
    from tests.test_gpu_occupancy import dilate_np
    rx, ry, rz = 512, 512, 257
    assert rx // 32 * ry * rz == G.SHAPED["occupancy_dilate_kernel"] > G.reach(G.row("occupancy_dilate_kernel"))
    gen = torch.Generator().manual_seed(751)
    mask = torch.rand((rz, ry, rx), generator=gen) < 0.01
    grid = N.OccupancyGrid.from_mask(mask, -4.0, 4.0).to("cuda")
    got = grid.dilate(1).to_mask().cpu()
    want = torch.from_numpy(dilate_np(mask.numpy()))
    assert mask[-1].any() and 0.1 < want.float().mean() < 0.4
    assert torch.equal(got, want)


@pytest.mark.parametrize("kind", ["adam", "clipped-adamw", "clipped-adam"])
def test_adam_on_the_second_trip(L, kind):
    """nrf_adam_step and nrf_adamw_step_loss (clipped; decoupled and not) at n = 1 048 576 + 300, two steps, against torch.optim on
    the CPU at test_clipped_update_matches_torch's 1e-6; the parameters past the first trip are copies of parameters 0 ...."""
    lib, st = L.lib(), L.stream_ptr()
    kernel = "adam_kernel<false>" if kind == "adam" else "adam_kernel<true>"
    n, cap = G.size(kernel), G.reach(G.row(kernel))
    decoupled, clipped = kind == "clipped-adamw", kind != "adam"
    wd = 1e-2 if decoupled else 1e-6
    p0 = dup(u01(761, n) - 0.5, cap)
    ref = torch.nn.Parameter(p0.clone())
    opt = (torch.optim.AdamW if decoupled else torch.optim.Adam)([ref], lr=5e-4, weight_decay=wd)
    p = p0.clone().cuda()
    m, v = torch.zeros_like(p), torch.zeros_like(p)
    ws = torch.empty(lib.nrf_grad_sqnorm_workspace_bytes(n) // 4, device="cuda")
    norm = torch.empty((), device="cuda")
    norms = []
    for step in (1, 2):
        g = dup(u01(762 + step, n) - 0.5, cap) * (10.0 ** (3 * step - 6))            # norms ~0.3 and ~300: on both sides of max_norm
        ref.grad = g.clone()
        if clipped:
            norms.append(float(torch.nn.utils.clip_grad_norm_([ref], 1.0)))
        opt.step()
        gd = g.cuda()
        if clipped:
            L.check(lib.nrf_grad_sqnorm_partials(L.ptr(gd), n, L.ptr(ws), ws.numel() * 4, st))
            L.check(lib.nrf_adamw_step_loss(L.ptr(p), L.ptr(gd), L.ptr(m), L.ptr(v), n, 5e-4, 0.9, 0.999, 1e-8, wd, step, int(decoupled), 1.0, L.ptr(ws),
                                            L.ptr(norm), None, 0, 1, 0.0, 0.0, 0.0, None, st))
            assert abs(norm.item() - norms[-1]) <= 1e-5 * norms[-1]
        else:
            L.check(lib.nrf_adam_step(L.ptr(p), L.ptr(gd), L.ptr(m), L.ptr(v), n, 5e-4, 0.9, 0.999, 1e-8, wd, step, st))
    torch.cuda.synchronize()
    assert not clipped or (norms[0] < 1.0 < norms[1])
    err = (p.cpu() - ref.detach()).abs().max().item()
    print(f"\nRECORD d {kind} n {n}: {err / 1e-6:.3f} of 1e-6")
    assert err < 1e-6
    for name, t in (("p", p), ("m", m), ("v", v)):
        same_tail(t, cap, name)


def test_repack_on_the_second_trip(N, L):
    """repack3_kernel is reached through a model's parameter count alone: a V3 model in the fp32 mode re-packs 1 851 232 work items
    (forward stream, backward stream, bias table), past 4096 x 256, so the tail of its backward stream and its bias table are the
    second trip.  test_device_repack_equals_host_pack's yardstick: weights loaded through the device path give the forward of a model
    that packed them on the host bit for bit, and its gradient within 1e-5 of the maximum (atomics: order only)."""
    from tests.test_gpu_training import make_v3, v3_inputs
    a, p = make_v3(N, "f32", scene="solid")
    b, _ = make_v3(N, "f32", scene="fog")
    pos, dirs, dino, g_rgb, g_den = (t.cuda() for t in v3_inputs(300))

    def grads(model):
        model.zero_grad(set_to_none=True)
        rgb, den = model.train()(pos, dirs, dino)
        ((rgb * g_rgb).sum() + (den * g_den).sum()).backward()
        return torch.cat([q.grad.reshape(-1) for q in model.parameters()])
    grads(b)                                                     # builds b's flat vector and training state
    items = sum(int(x) for x in stream_items(L, "v3", "f32"))
    assert items == G.SHAPED["repack3_kernel"] > G.reach(G.row("repack3_kernel"))
    with torch.no_grad():
        for name, t in b.state_dict().items():
            if name in p:
                t.copy_(p[name].cuda())
    b._gen += 1
    with torch.no_grad():
        ya, yb = a.eval()(pos, dirs, dino), b.eval()(pos, dirs, dino)
    assert torch.equal(ya[0], yb[0]) and torch.equal(ya[1], yb[1])
    assert rel_to_max(grads(b), grads(a)) < 1e-5


def stream_items(L, variant, mode):
    """Work items of one nrf_model_update_device launch for `mode`: forward stream, backward stream (pairs in the 16-bit modes) and the
    bias table, from the host-side packers."""
    shapes = O.layer_shapes(variant)
    arr, keep = (L.nrf_linear * len(shapes))(), []
    for i, (_, o, k) in enumerate(shapes):
        w, b = np.zeros((o, k), np.float32), np.zeros(o, np.float32)
        keep += [w, b]
        arr[i] = L.nrf_linear(w.ctypes.data_as(L.c_float_p), b.ctypes.data_as(L.c_float_p), o, k)
    arch = L.nrf_arch({"v1": 1, "v2": 2, "v3": 3}[variant], 12 if variant == "v3" else 10, 4, 256, 8, 64 if variant == "v3" else 0)
    ns, nb, nw = C.c_int64(), C.c_int64(), C.c_int64()
    L.check(L.lib().nrf_debug_pack(C.byref(arch), arr, len(shapes), L.MMA_MODES[mode], None, 0, C.byref(ns), None, 0, C.byref(nb)))
    L.check(L.lib().nrf_debug_pack_backward(C.byref(arch), arr, len(shapes), L.MMA_MODES[mode], None, 0, C.byref(nw)))
    per = 4                                                      # bytes per work item: one fp32 value, or a pair of 16-bit ones
    return ns.value // per, nw.value // per, nb.value


# ---------------------------------------------------------------------------------------------
# e. resampling and the hierarchical entries
# ---------------------------------------------------------------------------------------------
def pdf_waves(S, Ni):
    """sample_pdf_grid's wave count, restated (tests/test_launch_geometry_host.py holds the constants to the source)."""
    row_bytes, waves = (3 * S + 3 * Ni + 1) * 4, 4
    while waves > 1 and waves * row_bytes > 60 * 1024:
        waves >>= 1
    assert waves * row_bytes <= 60 * 1024
    return waves


@pytest.mark.parametrize("R,S,Ni,waves", [(G.size("sample_pdf_kernel"), 8, 8, 4), (9, 1300, 64, 2), (9, 2600, 64, 1)])
def test_resampling_past_the_grid_and_in_the_narrow_geometries(N, R, S, Ni, waves):
    """nrf_sample_pdf and nrf_sample_pdf_sorted with `u` given: the ray stride (4096 workgroups x 4 waves) at R = 16 389, and the
    2-wave and 1-wave workgroups of long LDS rows at R = 9 (more rays than waves: the stride runs there too).  The oracle at
    test_sample_pdf_vs_oracle's 1e-4, on its kind of weights (uniform plus one heavy bin); the oracle in float32 against a float64
    restatement stays within 4.5e-5 / 1.7e-6 / 1.3e-6 on these three inputs."""
    from nerf_few_shot_limitations_amd.ray_sampler import sample_pdf_sorted
    from tests.test_gpu_parity import TOL, maxdiff
    assert pdf_waves(S, Ni) == waves and G.size("sample_pdf_kernel") == G.size("sample_pdf_sorted_kernel")
    cap = G.reach(G.row("sample_pdf_kernel")) if R > 1000 else R - 4
    z = O.z_steps(2.0, 6.0, S).expand(R, S).contiguous()
    w = torch.from_numpy(O.uniform01(3, R * S).reshape(R, S)).clone()
    w[:, S // 3] += 5.0
    u = torch.from_numpy(O.uniform01(4, R * Ni).reshape(R, Ni)).clone()
    w, u = dup(w, cap), dup(u, cap)
    smp, union = N.sample_pdf(z, w, Ni, u=u)
    osmp, ounion = O.sample_pdf(z, w, Ni, u=u)
    e = max(maxdiff(smp, osmp), maxdiff(union, ounion))
    print(f"\nRECORD e sample_pdf R {R} S {S} Ni {Ni} ({waves} waves): {e / TOL:.3f} of 1e-4")
    assert e <= TOL and torch.all(union[:, 1:] >= union[:, :-1])
    srt = sample_pdf_sorted(z, w, Ni, u=u)
    assert torch.equal(srt, torch.sort(smp, dim=-1).values)      # the same samples, ascending
    assert torch.equal(torch.sort(torch.cat([z.cuda(), srt], -1), -1).values, union)
    for name, t in (("samples", smp), ("union", union), ("sorted", srt)):
        same_tail(t, cap, name)
    again = N.sample_pdf(z, w, Ni, u=u)
    assert torch.equal(again[0], smp) and torch.equal(again[1], union)


@pytest.mark.parametrize("layout", ["v1", "v2"])
def test_hier_loss_backward_on_the_second_trip(N, layout):
    """nrf_composite_hier_loss_backward at R = 65 573, S + Ni = 40 + 25: 4.26 M samples of the union, past 16 384 x 256 for
    merge_gather_kernel and scatter_add_kernel (and the wave-per-ray loss kernel on its second trip at M = 65).
    test_entry_equals_the_parents_kernels_on_the_gathered_union's yardstick: a stable sort plus the parent's kernels, bit for bit,
    with planted ties in the first ray and in the last."""
    from nerf_few_shot_limitations_amd.ray_sampler import sample_pdf_sorted
    from tests.test_gpu_hier_train import _mse_backward, _run_entry, _weights
    R, S, Ni = R_RAYS, 40, 25
    assert R * (S + Ni) == G.SHAPED["merge_gather_kernel"] > G.reach(G.row("merge_gather_kernel")) == G.reach(G.row("scatter_add_kernel"))
    white, wc, wf, seed = 1, 0.35, 0.7, 2000
    rgb_c, rgb_n = u01(seed, R, S, 3).cuda(), u01(seed + 1, R, Ni, 3).cuda()
    sig_c, sig_n = (u01(seed + 2, R, S) * 3 - 0.5).cuda(), (u01(seed + 3, R, Ni) * 3 - 0.5).cuda()
    sig_c[1, S // 2] = 1e6
    sig_c[2], sig_n[2] = -sig_c[2].abs(), -sig_n[2].abs()
    z_c = torch.sort(u01(seed + 4, R, S) * 4 + 2, dim=-1).values.cuda().contiguous()
    _, d = ray_batch(R, seed=seed + 5)
    tgt = u01(seed + 8, R, 3).cuda()
    z_n = sample_pdf_sorted(z_c, _weights(rgb_c, sig_c, z_c, d, 0), Ni).clone()
    for r in (0, R - 1):                                         # two equal new depths, and a new depth equal to an interior coarse one
        z_n[r, 1] = z_n[r, 0]
        z_n[r, Ni // 2] = z_c[r, S // 2]
        z_n[r] = torch.sort(z_n[r]).values
    assert bool((z_n[:, 1:] >= z_n[:, :-1]).all())
    zu, idx = torch.sort(torch.cat([z_c, z_n], 1), dim=1, stable=True)
    g_rgb = torch.gather(torch.cat([rgb_c, rgb_n], 1), 1, idx[..., None].expand(-1, -1, 3)).contiguous()
    g_sig = torch.gather(torch.cat([sig_c, sig_n], 1), 1, idx).contiguous()
    c = dict(R=R, rgb_c=rgb_c, rgb_n=rgb_n, sig_c=sig_c, sig_n=sig_n, z_c=z_c, z_n=z_n.contiguous(), d=d, tgt=tgt, zu=zu.contiguous())
    pred_c, d_rgb_c, d_sig_c, se_c = _mse_backward(rgb_c, sig_c, z_c, d, tgt, white, wc)
    pred_f, dg_rgb, dg_sig, se_f = _mse_backward(g_rgb, g_sig, c["zu"], d, tgt, white, wf)
    w_f = _weights(g_rgb, g_sig, c["zu"], d, white)
    back_rgb = torch.zeros_like(dg_rgb).scatter_(1, idx[..., None].expand(-1, -1, 3), dg_rgb)
    back_sig = torch.zeros_like(dg_sig).scatter_(1, idx, dg_sig)
    wc32, wf32 = torch.tensor(wc, dtype=torch.float32, device="cuda"), torch.tensor(wf, dtype=torch.float32, device="cuda")
    want = dict(pred_c=pred_c, pred_f=pred_f, parts=torch.stack([se_c, se_f]), ray_loss=wc32 * se_c + wf32 * se_f, zu=c["zu"], w=w_f,
                d_rgb_c=d_rgb_c + back_rgb[:, :S], d_sig_c=d_sig_c + back_sig[:, :S], d_rgb_n=back_rgb[:, S:], d_sig_n=back_sig[:, S:])
    zero = torch.ones(1000, device="cuda")
    got = _run_entry(c, S, Ni, layout == "v1", white, wc, wf, zero)
    for k, v in want.items():
        assert torch.isfinite(v).all(), k
        assert torch.equal(got[k], v), (k, float((got[k] - v).abs().max()))
    assert float(zero.abs().max()) == 0.0
    assert float(want["d_rgb_n"][R - 1].abs().max()) > 0 and float(se_f.min()) > 0


def test_composite_merge_on_the_second_trip(L):
    """nrf_composite_merge is one THREAD per ray, 16 384 x 256 of them per trip: its second trip starts at ray 4 194 304 (not at
    65 536 as for the wave-per-ray kernels), so R = 4 194 341 with S + Ni = 2 + 1.  (i) the merge of the two lists equals the same
    kernel on the stable-sorted union with Ni = 0, bit for bit, ties planted (coarse first among equals); (ii) rays past the first
    trip are copies of rays 0 ...; (iii) the fp32 oracle on the union at the render bar of 1e-4 (test_hierarchical_render_c3)."""
    row = G.row("composite_merge_kernel<false>")
    R, cap, S, Ni = G.size("composite_merge_kernel<false>"), G.reach(row), 2, 1
    gen = torch.Generator().manual_seed(771)
    rnd = lambda *s: torch.rand(s, generator=gen)
    z_c = torch.sort(rnd(R, S) * 4 + 2, dim=-1).values
    z_n = rnd(R, Ni) * 4 + 2
    z_n[::7, 0] = z_c[::7, 1]                                    # ties with a coarse depth
    raw_c, raw_n = rnd(R, S, 4) * 4 - 1.5, rnd(R, Ni, 4) * 4 - 1.5
    d = torch.nn.functional.normalize(rnd(R, 3) - 0.5, dim=-1) * (0.5 + rnd(R, 1))
    z_c, z_n, raw_c, raw_n, d = (dup(t, cap).cuda().contiguous() for t in (z_c, z_n, raw_c, raw_n, d))
    assert cap % 7 != 0 and bool((z_n[cap:, 0] == z_c[cap:, 1]).any())

    def merge(zc, rc, zn, rn, ni):
        U = zc.shape[1] + ni
        o = dict(rgb=torch.full((R, 3), float("nan"), device="cuda"), depth=torch.full((R,), float("nan"), device="cuda"),
                 w=torch.full((R, U), float("nan"), device="cuda"), zu=torch.full((R, U), float("nan"), device="cuda"))
        L.check(L.lib().nrf_composite_merge(L.ptr(zc), L.ptr(rc), L.ptr(zn) if ni else None, L.ptr(rn) if ni else None, L.ptr(d), R, zc.shape[1], ni,
                                            L.MMA_MODES["f32"], 1, 0, L.ptr(o["rgb"]), L.ptr(o["depth"]), L.ptr(o["w"]), L.ptr(o["zu"]), L.stream_ptr()))
        torch.cuda.synchronize()
        return o
    got = merge(z_c, raw_c, z_n, raw_n, Ni)
    zu, idx = torch.sort(torch.cat([z_c, z_n], 1), dim=1, stable=True)
    rows = torch.gather(torch.cat([raw_c, raw_n], 1), 1, idx[..., None].expand(-1, -1, 4)).contiguous()
    one = merge(zu.contiguous(), rows, None, None, 0)
    for k in ("rgb", "depth", "w", "zu"):
        assert torch.isfinite(got[k]).all() and torch.equal(got[k], one[k]), k
        same_tail(got[k], cap, k)
    assert torch.equal(got["zu"], zu)
    rc = rows.cpu()
    o_rgb, o_dep, o_w = O.volume_render(torch.sigmoid(rc[..., :3]), rc[..., 3:4], zu.cpu(), d.cpu(), white_bkgd=True)
    e = (float((got["rgb"].cpu() - o_rgb).abs().max()), float((got["depth"].cpu() - o_dep).abs().max()), float((got["w"].cpu() - o_w).abs().max()))
    print(f"\nRECORD a composite_merge R {R}: rgb {e[0] / 1e-4:.3f} depth {e[1] / 1e-4:.3f} weights {e[2] / 1e-4:.3f} of 1e-4")
    assert max(e) <= 1e-4


# ---------------------------------------------------------------------------------------------
# f. the training chain past 2^32 context bytes and into the weight gradient's two-round grid
# ---------------------------------------------------------------------------------------------
def chain(L, model, net, inputs, g, ctx=None):
    """One saving forward + backward through the C ABI on the first len(g[0]) rows of `inputs`: (outputs, flat gradient).
    net v1: inputs (x_enc,), g (d_out4,); v3: inputs (pos, dirs, dino), g (d_rgb, d_density)."""
    from nerf_few_shot_limitations_amd.training import _train_handle
    lib, st, dev = L.lib(), L.stream_ptr(), torch.device("cuda", 0)
    h, mode = _train_handle(model, dev)
    n = g[0].shape[0]
    nbytes = lib.nrf_train_context_bytes(h, mode, n)
    buf = ctx if ctx is not None else torch.empty(nbytes, dtype=torch.uint8, device=dev)
    assert buf.numel() >= nbytes > 0
    cb = C.c_void_p(buf.data_ptr())
    grad = torch.zeros(model.flat_params().flat.numel(), device=dev)
    if net == "v1":
        out = (torch.empty((n, 4), device=dev),)
        L.check(lib.nrf_mlp_forward_train_v1(h, mode, L.ptr(inputs[0]), n, L.ptr(out[0]), cb, nbytes, st))
        L.check(lib.nrf_mlp_backward_v1(h, mode, L.ptr(out[0]), L.ptr(g[0]), n, cb, nbytes, L.ptr(grad), st))
    else:
        out = (torch.empty((n, 3), device=dev), torch.empty((n, 1), device=dev))
        L.check(lib.nrf_mlp_forward_train(h, mode, *[L.ptr(t) for t in inputs], n, L.ptr(out[0]), L.ptr(out[1]), cb, nbytes, st))
        L.check(lib.nrf_mlp_backward(h, mode, L.ptr(out[0]), L.ptr(out[1]), L.ptr(g[0]), L.ptr(g[1]), n, cb, nbytes, L.ptr(grad), st))
    torch.cuda.synchronize()
    return out, grad


def inference(L, model, net, inputs, n):
    from nerf_few_shot_limitations_amd.training import _train_handle
    h, mode = _train_handle(model, torch.device("cuda", 0))
    if net == "v1":
        out = (torch.empty((n, 4), device="cuda"),)
        L.check(L.lib().nrf_mlp_forward_v1(h, mode, L.ptr(inputs[0]), n, L.ptr(out[0]), L.stream_ptr()))
    else:
        out = (torch.empty((n, 3), device="cuda"), torch.empty((n, 1), device="cuda"))
        L.check(L.lib().nrf_mlp_forward(h, mode, *[L.ptr(t) for t in inputs], n, L.ptr(out[0]), L.ptr(out[1]), L.stream_ptr()))
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("net,mode", [("v1", "f32"), ("v1", "bf16"), ("v3", "bf16")])
def test_training_chain_past_4_gib_of_context_and_in_the_two_round_weight_gradient(N, L, net, mode):
    """The saving forward, the backward chain and the weight gradient at the smallest batch (a multiple of 1000) with
    tiles32(n) >= 8192 -- wgrad_grid's two rounds of workgroups, another slab partition, a longer reduce -- whose context, partial sums
    included, passes 2^32 bytes: byte offsets into the context that no 32-bit value holds.  The incoming gradient is exactly zero
    except on three windows (the first 512 samples, 512 around n / 2, the last 300: ragged), so the gradient must be the sum of the
    three windows run alone at their own small n -- runs that test_gradients_fp32_mode_match_autograd and the stage tests tie to
    autograd and to the rounding model -- within rel_to_max < 2e-5, test_gradient_is_additive_over_the_batch_at_scale's figure for
    the same comparison, in both modes.  Also: two runs give equal bits, the saving forward's outputs are the inference forward's, and
    in fp32 halving g halves the gradient exactly."""
    from nerf_few_shot_limitations_amd.training import _train_handle
    from tests.test_gpu_training import make_model, make_v3
    model = (make_model(N, mode, scene="solid") if net == "v1" else make_v3(N, mode, scene="solid"))[0]
    h, m = _train_handle(model, torch.device("cuda", 0))
    tiles_min = G.cap(G.row("weight_grad_reduce_kernel"))
    tiles32 = lambda k: (k + 255) // 256 * 8
    n = 1000
    while tiles32(n) < tiles_min or L.lib().nrf_train_context_bytes(h, m, n) <= 2 ** 32:
        n += 1000
    nbytes = L.lib().nrf_train_context_bytes(h, m, n)
    assert tiles32(n) >= tiles_min and nbytes > 2 ** 32
    assert tiles32(n - 1000) < tiles_min or L.lib().nrf_train_context_bytes(h, m, n - 1000) <= 2 ** 32
    print(f"\nRECORD f {net} {mode}: n {n}, tiles32 {tiles32(n)}, context {nbytes} bytes")
    gen = torch.Generator(device="cuda").manual_seed(900)
    rnd = lambda *s: torch.rand(s, generator=gen, device="cuda")
    if net == "v1":
        inputs = (N.PositionalEncoding(10)(rnd(n, 3) * 4 - 2).contiguous(),)
        g = (rnd(n, 4) - 0.5,)
    else:
        inputs = (rnd(n, 3) * 4 - 2, torch.nn.functional.normalize(rnd(n, 3) - 0.5, dim=-1).contiguous(), rnd(n, 64) * 2 - 1)
        g = (rnd(n, 3) - 0.5, rnd(n, 1) - 0.5)
    windows = [(0, 512), (n // 2 - 256, n // 2 + 256), (n - 300, n)]
    live = torch.zeros(n, 1, device="cuda")
    for a, b in windows:
        live[a:b] = 1.0
    g = tuple((t * live).contiguous() for t in g)
    ctx = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    out, full = chain(L, model, net, inputs, g, ctx)
    out2, again = chain(L, model, net, inputs, g, ctx)
    assert torch.equal(full, again) and all(torch.equal(x, y) for x, y in zip(out, out2))
    for x, y in zip(out, inference(L, model, net, inputs, n)):
        assert torch.equal(x, y)
    if mode == "f32":
        _, half = chain(L, model, net, inputs, tuple(0.5 * t for t in g), ctx)
        assert torch.equal(half * 2, full)
    del ctx
    parts = torch.zeros_like(full)
    for a, b in windows:
        _, gw = chain(L, model, net, tuple(t[a:b].contiguous() for t in inputs), tuple(t[a:b].contiguous() for t in g))
        parts += gw
    e = rel_to_max(parts, full)
    print(f"RECORD f {net} {mode}: sum of the three windows against the full batch: {e / 2e-5:.3f} of 2e-5")
    assert full.abs().max() > 0 and e < 2e-5
