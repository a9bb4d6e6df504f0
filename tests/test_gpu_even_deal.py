"""The even deal of a launch's rays to the workgroups (csrc/ray_deal.hpp; render_march) must be invisible: a frame rendered with it
equals, bit for bit, the same frame under the uniform deal pinned by NRF_SPW (read per launch) at one sample per column and pass
(NRF_SPW=0) and at eight (NRF_SPW=3) -- whole frames, a ragged ray count with jitter and the weights / depths, the hold + tail pair
and a two-view tile job, in the 64-column (f16) and 32-column (f32) geometries."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import nerf_oracle as O

pytestmark = pytest.mark.gpu

H = W = 400           # 160 000 rays: 625 units of 4 rays per workgroup and a remainder on 256 compute units
S = 32


def T(a):
    return torch.from_numpy(np.asarray(a))


@pytest.fixture(scope="module")
def N():
    import nerf_few_shot_limitations_amd as N
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from nerf_few_shot_limitations_amd import _lib
    _lib.lib()
    return N


def model_v1(N, mode):
    m = N.NeRFMLP(pos_dim=63, hidden_dim=256, n_layers=8, mma_mode=mode)
    m.load_state_dict(O.make_weights("v1", 0, "solid"))
    return m.cuda().eval()


def deal_is_even(n_rays, n_samples, cols):
    """What the launcher picks for this launch on this device (the environment as it is now)."""
    from nerf_few_shot_limitations_amd import _lib as L
    head = (C.c_int64 * 4)()
    n = C.c_int64(0)
    cu = torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count
    L.check(L.lib().nrf_debug_ray_deal(n_rays, n_samples, cols, cu, head, None, 0, C.byref(n)))
    return bool(head[0])


def under_each_deal(monkeypatch, render, n_rays, n_samples, cols):
    """render() under the launcher's own (even) deal, then under the uniform deal at SPW = 1 and SPW = 8."""
    monkeypatch.delenv("NRF_SPW", raising=False)
    assert deal_is_even(n_rays, n_samples, cols), "the case was chosen so that the launcher takes the even deal"
    out = [render()]
    for l in ("0", "3"):
        monkeypatch.setenv("NRF_SPW", l)
        assert not deal_is_even(n_rays, n_samples, cols)
        out.append(render())
    monkeypatch.delenv("NRF_SPW")
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("mode,cols", [("f16", 64), ("f32", 32)])
def test_even_deal_frame_equals_the_uniform_deals(N, mode, cols, monkeypatch):
    c2w = T(O.LEGO_LIKE_C2W)
    m = model_v1(N, mode)
    even, spw1, spw8 = under_each_deal(monkeypatch, lambda: N.render_camera(m, H, W, O.focal_for(W), c2w, 2.0, 6.0, S), H * W, S, cols)
    for other in (spw1, spw8):
        assert torch.equal(even[0], other[0]) and torch.equal(even[1], other[1])
    assert torch.isfinite(even[0]).all() and float(even[0].max()) > 0.05           # a frame, not zeros


@pytest.mark.parametrize("mode,cols", [("f16", 64), ("f32", 32)])
def test_ragged_ray_count_with_jitter_weights_and_depths(N, mode, cols, monkeypatch):
    """159 997 rays: the last unit of 4 rays is ragged, and so is the last workgroup's range."""
    c2w = T(O.LEGO_LIKE_C2W)
    m = model_v1(N, mode)
    ro, rd = N.get_rays(H, W, O.focal_for(W), c2w)
    ro, rd = ro.reshape(-1, 3)[: H * W - 3].contiguous(), rd.reshape(-1, 3)[: H * W - 3].contiguous()
    n = ro.shape[0]
    even, spw1, spw8 = under_each_deal(monkeypatch, lambda: N.render_rays(m, ro, rd, 2.0, 6.0, S, perturb=True, seed=5, return_z=True), n, S, cols)
    for other in (spw1, spw8):
        for k in ("rgb", "depth", "weights", "z_vals"):
            assert even[k].shape[0] == n and torch.equal(even[k], other[k]), (mode, k)


def test_hold_and_tail_pair(N, monkeypatch):
    """Tail mode: the prefix launch marches S samples of S + 1 under the even deal, the tail launch the last one."""
    c2w = T(O.LEGO_LIKE_C2W)
    m = model_v1(N, "f16")
    even, spw1, spw8 = under_each_deal(monkeypatch, lambda: N.render_camera(m, H, W, O.focal_for(W), c2w, 2.0, 6.0, S + 1, tail_mode="f16x3"),
                                       H * W, S, 64)
    for other in (spw1, spw8):
        assert torch.equal(even[0], other[0]) and torch.equal(even[1], other[1])


def test_two_view_tile_job(N, monkeypatch):
    """One launch of two views' tiles (rank 0 of 2, 20-row tiles: 2 x 80 000 rays through global_ray) with jitter."""
    from nerf_few_shot_limitations_amd import tiles
    c2w = T(O.LEGO_LIKE_C2W)
    poses = torch.stack([c2w, c2w.clone()])
    poses[1, 0, 3] += 0.2
    m = model_v1(N, "f16")
    tile_rays = 20 * W

    def render():
        job = tiles.TileJob(m, H, W, O.focal_for(W), poses, 2.0, 6.0, S, 0, 2, tile_rays, perturb=True, seed=777)
        assert job.launches_per_step == 1 and job.rays_per_launch == H * W
        job.launch()
        return job.buf.clone()

    even, spw1, spw8 = under_each_deal(monkeypatch, render, H * W, S, 64)
    assert torch.equal(even, spw1) and torch.equal(even, spw8)
    assert float(even[..., :3].max()) > 0.05 and not torch.equal(even[0], even[1])
