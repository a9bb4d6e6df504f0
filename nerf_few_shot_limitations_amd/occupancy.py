"""Occupancy bit grids for empty-space skipping (include/nerfhip.h: nrf_occupancy).

An `OccupancyGrid` holds one bit per cell of an axis-aligned box: bit ((iz * ry + iy) * rx + ix) of the word array, 32 cells per
word, 1 = occupied.  The render entry points that take `occupancy=` (renderer.py, tiles.py) step over every sample whose cell is
empty; a skipped sample is composited as density 0.  `from_model` builds a grid by probing the network's density at a few points
per cell (nrf_occupancy_pack) and growing the result by one cell (nrf_occupancy_dilate): it is NOT conservative between the
probed points, which is why skipping is opt-in.  `from_views` / `prune` build a grid from what the training views render instead
(nrf_occupancy_mark_camera): a cell stays when a sample of weight > weight_threshold fell into it (hit), or -- by default -- when no
marking ray reached it with transmittance > seen_eps (not seen: behind a surface or outside every frustum, where a held-out view
may look).  Grids over the same box combine with `&`, `|` and `~`.

Training under a grid (training.FusedStep.step_rays / step_view with occupancy=) needs a grid that follows the field while it
moves: `full` is the all-ones grid a run starts from, `refresh` re-probes a slab of cells per call and keeps a decaying maximum of
the densities it has seen per cell.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _lib as L


def _triple(v, what):
    t = tuple(float(x) for x in (v if hasattr(v, "__len__") else (v, v, v)))
    if len(t) != 3:
        raise ValueError(f"{what} must be a number or three numbers (x, y, z)")
    return t


def _counter_u01(seed, index):
    """U[0,1) from (seed, int64 tensor of counters): a 32-bit integer hash (the murmur3 finaliser) evaluated in int64, identical on
    every device; 24 random bits."""
    m = 0xFFFFFFFF
    h = (index + (int(seed) & 0x7FFFFFFF) * 0x9E3779B1) & m
    h = ((h ^ (h >> 16)) * 0x85EBCA6B) & m
    h = ((h ^ (h >> 13)) * 0xC2B2AE35) & m
    h = h ^ (h >> 16)
    return (h >> 8).to(torch.float32) * (1.0 / 16777216.0)


class OccupancyGrid:
    def __init__(self, bits, res, lo, hi, outside=0):
        """bits: int32 tensor of rx*ry*rz/32 words; res = (rx, ry, rz); lo / hi: the box; outside: what happens to a sample
        outside the box (0: it is evaluated, 1: it is skipped)."""
        self.res = tuple(int(r) for r in res)
        rx, ry, rz = self.res
        if len(self.res) != 3 or not all(1 <= r <= 512 for r in self.res) or rx % 32:
            raise ValueError("res = (rx, ry, rz): each in 1..512 and rx a multiple of 32")
        self.lo, self.hi = _triple(lo, "lo"), _triple(hi, "hi")
        if not all(np.isfinite(a) and np.isfinite(b) and b > a for a, b in zip(self.lo, self.hi)):
            raise ValueError("need finite lo < hi on every axis")
        if outside not in (0, 1):
            raise ValueError("outside must be 0 (evaluate) or 1 (skip)")
        self.outside = int(outside)
        if bits.dtype != torch.int32 or bits.numel() != rx * ry * rz // 32:
            raise ValueError("bits must be an int32 tensor of rx*ry*rz/32 words")
        self.bits = bits.contiguous().reshape(-1)

    # ---- geometry ---------------------------------------------------------------------------------
    @property
    def scale(self):
        """Cells per unit length as the kernels get them: float32(res) / (float32(hi) - float32(lo))."""
        lo, hi = np.asarray(self.lo, np.float32), np.asarray(self.hi, np.float32)
        return tuple(float(v) for v in (np.asarray(self.res, np.float32) / (hi - lo)))

    @property
    def n_cells(self):
        return self.res[0] * self.res[1] * self.res[2]

    def to(self, device):
        g = OccupancyGrid(self.bits.to(device), self.res, self.lo, self.hi, self.outside)
        ema = getattr(self, "ema", None)
        if ema is not None:                                           # a refreshed grid keeps its per-cell values and its place in the round
            g.ema, g._cursor, g._refreshes = ema.to(device), self._cursor, self._refreshes
        return g

    # ---- algebra: bitwise operations on the words, on whatever device they live -------------------------
    def _like(self, bits):
        return OccupancyGrid(bits, self.res, self.lo, self.hi, self.outside)

    def _same_cells(self, other):
        if not isinstance(other, OccupancyGrid):
            raise TypeError("an OccupancyGrid combines with an OccupancyGrid")
        if (self.res, self.lo, self.hi, self.outside) != (other.res, other.lo, other.hi, other.outside):
            raise ValueError("grids combine only over the same res, box (lo, hi) and outside")
        return other.bits.to(self.bits.device)

    def __and__(self, other):
        return self._like(torch.bitwise_and(self.bits, self._same_cells(other)))

    def __or__(self, other):
        return self._like(torch.bitwise_or(self.bits, self._same_cells(other)))

    def __invert__(self):
        return self._like(torch.bitwise_not(self.bits))

    # ---- masks ------------------------------------------------------------------------------------
    @classmethod
    def full(cls, res, lo, hi, outside=0, device=None):
        """The all-ones grid of res = (rx, ry, rz) (or one number) cells over [lo, hi]: every sample is evaluated.  What a training
        run under a grid starts from (and returns to when it is resumed), before `refresh` has seen the field."""
        res = tuple(int(r) for r in (res if hasattr(res, "__len__") else (res,) * 3))
        if len(res) != 3 or not all(1 <= r <= 512 for r in res) or res[0] % 32:
            raise ValueError("res = (rx, ry, rz): each in 1..512 and rx a multiple of 32")
        bits = torch.full((res[0] * res[1] * res[2] // 32,), -1, dtype=torch.int32, device=device if device is not None else "cpu")
        return cls(bits, res, lo, hi, outside)

    @classmethod
    def from_mask(cls, mask, lo, hi, outside=0):
        """mask: bool tensor (rz, ry, rx), True = occupied."""
        mask = torch.as_tensor(mask)
        if mask.dim() != 3:
            raise ValueError("mask must be (rz, ry, rx)")
        rz, ry, rx = (int(v) for v in mask.shape)
        if rx % 32:
            raise ValueError("rx (the last axis of the mask) must be a multiple of 32")
        sh = torch.arange(32, dtype=torch.int64, device=mask.device)
        words = (mask.reshape(-1, 32).to(torch.int64) << sh).sum(dim=1)
        words = torch.where(words >= 2 ** 31, words - 2 ** 32, words).to(torch.int32)        # the bit pattern of the uint32 word
        return cls(words, (rx, ry, rz), lo, hi, outside)

    def to_mask(self):
        rx, ry, rz = self.res
        sh = torch.arange(32, dtype=torch.int64, device=self.bits.device)
        return (((self.bits.to(torch.int64)[:, None] >> sh) & 1) != 0).reshape(rz, ry, rx)

    @property
    def occupied_fraction(self):
        return float(self.to_mask().to(torch.float32).mean())

    # ---- building ---------------------------------------------------------------------------------
    def dilate(self, n=1):
        """The grid grown by n cells in every direction (n passes of nrf_occupancy_dilate)."""
        L.require_gpu()
        if not self.bits.is_cuda:
            raise ValueError("dilate runs on the GPU: move the grid there first (grid.to(device))")
        cur = self.bits
        res = (C.c_int32 * 3)(*self.res)
        with torch.cuda.device(cur.device):
            for _ in range(int(n)):
                out = torch.empty_like(cur)
                L.check(L.lib().nrf_occupancy_dilate(cur.data_ptr(), res, out.data_ptr(), L.stream_ptr()))
                cur = out
        return OccupancyGrid(cur, self.res, self.lo, self.hi, self.outside)

    @staticmethod
    def cell_points(res, lo, hi, first_cell, n_cells, samples_per_cell, seed=0, device="cpu"):
        """(n_cells, samples_per_cell, 3) float32 points a build evaluates for cells first_cell .. first_cell + n_cells - 1 of a
        (rx, ry, rz) grid over [lo, hi]: sample 0 is the cell centre, sample j > 0 sits at counter-RNG offsets (seed, cell, j, axis)
        inside the cell.  Deterministic and the same on every device."""
        rx, ry, rz = (int(r) for r in res)
        lo, hi = _triple(lo, "lo"), _triple(hi, "hi")
        k = int(samples_per_cell)
        cell = torch.arange(int(first_cell), int(first_cell) + int(n_cells), dtype=torch.int64, device=device)
        idx = torch.stack([cell % rx, (cell // rx) % ry, cell // (rx * ry)], dim=-1)                       # (n, 3): ix, iy, iz
        j = torch.arange(k, dtype=torch.int64, device=device)
        ax = torch.arange(3, dtype=torch.int64, device=device)
        u = _counter_u01(seed, (cell[:, None, None] * k + j[None, :, None]) * 3 + ax[None, None, :])       # (n, k, 3)
        u[:, 0, :] = 0.5
        lo_t = torch.tensor(lo, dtype=torch.float32, device=device)
        size = (torch.tensor(hi, dtype=torch.float32, device=device) - lo_t) / torch.tensor([rx, ry, rz], dtype=torch.float32, device=device)
        return lo_t + (idx[:, None, :].to(torch.float32) + u) * size

    @staticmethod
    def _density(model, pts, dino):
        """Densities (n,) of `model` at points (n,3) through NeRFMLP.forward: V1 encodes and takes the raw sigma, V2 / V3 run with a
        fixed unit view direction (the density does not depend on it), V3 on the features of the source view `dino`."""
        dev = pts.device
        if model.net == L.NRF_NET_V1:
            n, pe = pts.shape[0], 3 * (2 * model.pos_freq + 1)
            enc = torch.empty((n, pe), dtype=torch.float32, device=dev)
            L.check(L.lib().nrf_encode(L.ptr(pts), n, 3, model.pos_freq, 1, None, L.ptr(enc), L.stream_ptr()))
            return model(enc)[:, 3]
        dirs = torch.zeros_like(pts)
        dirs[:, 2] = -1.0
        feats = None
        if model.net == L.NRF_NET_V3:
            from .renderer import make_dino
            d, keep = make_dino(**dino)
            feats = torch.empty((pts.shape[0], model.dino_dim), dtype=torch.float32, device=dev)
            L.check(L.lib().nrf_project_fetch(C.byref(d), L.ptr(pts), pts.shape[0], L.ptr(feats), None, L.stream_ptr()))
            del keep
        return model(pts, dirs, feats)[1].reshape(-1)

    @classmethod
    def from_model(cls, model, lo, hi, resolution=128, threshold=0.0, samples_per_cell=4, dilate=1, mma_mode=None, dino=None,
                   chunk_cells=1 << 18, seed=0, device=None, outside=0):
        """Probe `model`'s density at `samples_per_cell` points of every cell (cell_points), mark the cells whose maximum exceeds
        `threshold`, grow the result by `dilate` cells.  resolution: cells per axis (a number or (rx, ry, rz)).  A V3 grid belongs
        to ONE source view: dino=dict(features=, pose=, focal=, H=, W=) is required."""
        L.require_gpu()
        if model.net == L.NRF_NET_V3 and dino is None:
            raise ValueError("a use_dino model's density depends on the source view: from_model needs dino=dict(features=, pose=, focal=, H=, W=)")
        res = tuple(int(r) for r in (resolution if hasattr(resolution, "__len__") else (resolution,) * 3))
        grid = cls(torch.zeros((res[0] * res[1] * res[2] // 32,), dtype=torch.int32), res, lo, hi, outside)        # validates res / box
        if device is None:
            p = next(model.parameters())
            device = p.device if p.is_cuda else torch.device("cuda", torch.cuda.current_device())
        device = torch.device(device)
        k = int(samples_per_cell)
        if k < 1:
            raise ValueError("samples_per_cell must be >= 1")
        chunk = max(32, int(chunk_cells) // 32 * 32)
        bits = torch.empty((grid.n_cells // 32,), dtype=torch.int32, device=device)
        was_training, own_mode = model.training, model.mma_mode
        model.eval()
        if mma_mode is not None:
            model.mma_mode = mma_mode
        try:
            with torch.no_grad(), torch.cuda.device(device):
                for first in range(0, grid.n_cells, chunk):
                    n = min(chunk, grid.n_cells - first)
                    pts = cls.cell_points(res, lo, hi, first, n, k, seed, device).reshape(-1, 3).contiguous()
                    dens = cls._density(model, pts, dino).contiguous()
                    L.check(L.lib().nrf_occupancy_pack(L.ptr(dens), n, k, float(threshold), bits[first // 32:].data_ptr(), L.stream_ptr()))
        finally:
            model.mma_mode = own_mode
            model.train(was_training)
        grid = cls(bits, res, lo, hi, outside)
        return grid.dilate(dilate) if dilate else grid

    # ---- following a field that is being trained -----------------------------------------------------
    def refresh(self, model, decay=0.95, threshold=0.0, samples_per_cell=4, cells=None, seed=None, dino=None, mma_mode=None):
        """Re-probe one slab of the grid, in place, and return (first_cell, n_cells) of the slab.

        The grid keeps one fp32 value per cell (`ema`, zeros before the first refresh).  A call probes `model`'s density at
        `samples_per_cell` points (cell_points with `seed`) of each of `cells` contiguous cells -- a multiple of 32; default: the
        whole grid -- through the network itself (_density), sets

            ema[c] = max(decay * ema[c], max over the cell's probes)

        on that slab and re-packs the slab's bits as ema[c] > threshold (nrf_occupancy_pack; a NaN value is occupied).  Cells
        outside the slab keep their values and bits.  Slabs go round robin: the next call starts where this one ended, the last
        slab of a round is cut at the end of the grid, so every cell is visited exactly once every ceil(n_cells / cells) calls.
        seed=None takes the number of refreshes so far, so that a cell is probed at new points in every round.

        Probing the NETWORK -- not the weights the training rays render -- is what lets a cell come back that skipping starved of
        gradient: a skipped sample passes no gradient, so nothing a step under the grid computes could ever show that the field
        has grown into an empty cell; the density at the cell's probes does, and the decaying maximum keeps a cell occupied for a
        while after one probe found it dense.  A V3 grid belongs to ONE source view: dino=dict(features=, pose=, focal=, H=, W=)."""
        L.require_gpu()
        if not self.bits.is_cuda:
            raise ValueError("refresh runs on the GPU: move the grid there first (grid.to(device))")
        if model.net == L.NRF_NET_V3 and dino is None:
            raise ValueError("a use_dino model's density depends on the source view: refresh needs dino=dict(features=, pose=, focal=, H=, W=)")
        if not (0.0 <= float(decay) <= 1.0):
            raise ValueError("decay must be in [0, 1]")
        k = int(samples_per_cell)
        if k < 1:
            raise ValueError("samples_per_cell must be >= 1")
        n_cells = self.n_cells
        cells = n_cells if cells is None else int(cells)
        if cells < 32 or cells % 32:
            raise ValueError("cells must be a positive multiple of 32 (a slab starts and ends on a word of the bit array)")
        dev = self.bits.device
        if getattr(self, "ema", None) is None or self.ema.device != dev:
            old = getattr(self, "ema", None)
            self.ema = old.to(dev) if old is not None else torch.zeros((n_cells,), dtype=torch.float32, device=dev)
            self._cursor = getattr(self, "_cursor", 0)
            self._refreshes = getattr(self, "_refreshes", 0)
        first = self._cursor
        n = min(cells, n_cells - first)
        if seed is None:
            seed = self._refreshes
        was_training, own_mode = model.training, model.mma_mode
        model.eval()
        if mma_mode is not None:
            model.mma_mode = mma_mode
        try:
            with torch.no_grad(), torch.cuda.device(dev):
                pts = self.cell_points(self.res, self.lo, self.hi, first, n, k, seed, dev).reshape(-1, 3).contiguous()
                probe = self._density(model, pts, dino).reshape(n, k).max(dim=1).values
                slab = self.ema[first:first + n]
                slab.copy_(torch.maximum(slab * float(decay), probe))
                L.check(L.lib().nrf_occupancy_pack(L.ptr(slab), n, 1, float(threshold), self.bits[first // 32:].data_ptr(), L.stream_ptr()))
        finally:
            model.mma_mode = own_mode
            model.train(was_training)
        self._cursor = 0 if first + n >= n_cells else first + n
        self._refreshes += 1
        return first, n

    # ---- building from rendered weights -----------------------------------------------------------
    def _box_args(self):
        return (C.c_int32 * 3)(*self.res), (C.c_float * 3)(*self.lo), (C.c_float * 3)(*self.scale)

    @staticmethod
    def _mark_settings(weight_threshold, seen_eps):
        tau = float(weight_threshold)
        if not (np.isfinite(tau) and tau >= 0.0):
            raise ValueError("weight_threshold must be finite and >= 0")
        if seen_eps is not None and not (0.0 <= float(seen_eps) < 1.0):
            raise ValueError("seen_eps must be in [0, 1)")
        return tau, None if seen_eps is None else float(seen_eps)

    def _mark_words(self, words, what):
        """The word array a mark call ORs into: the caller's (checked) or a zeroed one on the grid's device."""
        if words is None:
            return torch.zeros_like(self.bits)
        if not (isinstance(words, torch.Tensor) and words.dtype == torch.int32 and words.is_contiguous() and words.device == self.bits.device
                and words.numel() == self.bits.numel()):
            raise ValueError(f"{what} must be a contiguous int32 tensor of rx*ry*rz/32 words on the grid's device")
        return words

    def mark(self, rays_o, rays_d, z_vals, weights, weight_threshold=0.0, seen_eps=None, hit=None, seen=None):
        """Mark this grid's cells from a render's per-sample outputs (nrf_occupancy_mark_rays): rays_o / rays_d (R,3), z_vals and
        weights (R,S) as render_rays(return_z=True) returns them.  Returns (hit, seen), int32 word tensors in the layout of `bits`:
        hit -- a sample with !(weight <= weight_threshold) fell into the cell; seen -- a sample fell into it while its ray still had
        transmittance 1 - sum(earlier weights) > seen_eps (seen_eps=None: not computed, `seen` is returned as it came).  hit= / seen=
        are accumulated into (OR); the grid's own bits play no part."""
        L.require_gpu()
        if not self.bits.is_cuda:
            raise ValueError("mark runs on the GPU: move the grid there first (grid.to(device))")
        tau, eps = self._mark_settings(weight_threshold, seen_eps)
        dev = self.bits.device
        w = L.dev_f32(weights, dev)
        z = L.dev_f32(z_vals, dev)
        if w.dim() != 2 or z.shape != w.shape or w.shape[1] < 1:
            raise ValueError("weights and z_vals must both be (R, S) with S >= 1")
        o, d = L.dev_f32(rays_o, dev).reshape(-1, 3), L.dev_f32(rays_d, dev).reshape(-1, 3)
        if o.shape[0] != w.shape[0] or d.shape[0] != w.shape[0]:
            raise ValueError("rays_o and rays_d must be (R, 3) for weights (R, S)")
        hit = self._mark_words(hit, "hit")
        if eps is not None:
            seen = self._mark_words(seen, "seen")
        res, lo, scale = self._box_args()
        with torch.cuda.device(dev):
            L.check(L.lib().nrf_occupancy_mark_rays(L.ptr(o), L.ptr(d), w.shape[0], w.shape[1], L.ptr(z), L.ptr(w), res, lo, scale, tau,
                                                    eps if eps is not None else 0.0, hit.data_ptr(), seen.data_ptr() if eps is not None else None,
                                                    L.stream_ptr()))
        return hit, seen

    def _view_marks(self, model, poses, H, W, focal, near, far, n_samples, weight_threshold=0.0, seen_eps=1e-2, base=None, mma_mode=None,
                   dino=None, lindisp=False, chunk_rays=1 << 16):
        """(hit, seen) word tensors of this grid's cells over the views `poses` ((n,4,4) or one (4,4) camera-to-world): every view is
        rendered through the camera route in ray ranges of `chunk_rays` -- unjittered, ert_eps = 0, in `mma_mode`, under
        occupancy=base when a base grid is given -- with weights and z_vals requested, and each range is marked by
        nrf_occupancy_mark_camera.  seen_eps=None: seen is not computed (None)."""
        from .ray_sampler import _c2w12
        from .renderer import _handle, _opts, make_dino
        L.require_gpu()
        if not self.bits.is_cuda:
            raise ValueError("marking runs on the GPU: move the grid there first (grid.to(device))")
        tau, eps = self._mark_settings(weight_threshold, seen_eps)
        if model.net == L.NRF_NET_V3 and dino is None:
            raise ValueError("a use_dino model's weights depend on the source view: marking needs dino=dict(features=, pose=, focal=, H=, W=)")
        poses = torch.as_tensor(poses).detach().to("cpu", torch.float32)
        poses = poses.reshape(1, *poses.shape) if poses.dim() == 2 else poses
        H, W, S = int(H), int(W), int(n_samples)
        chunk = max(1, min(int(chunk_rays), H * W))
        dev = self.bits.device
        mode = mma_mode or model.mma_mode
        hit = torch.zeros_like(self.bits)
        seen = torch.zeros_like(self.bits) if eps is not None else None
        res, lo, scale = self._box_args()
        was_training = model.training
        model.eval()
        try:
            with torch.no_grad(), torch.cuda.device(dev):
                dn, keep = make_dino(**dino) if model.net == L.NRF_NET_V3 else (None, None)
                opts = _opts(near, far, S, False, None, None, lindisp, 0.0, False, mode, dn, dev)
                h = _handle(model, dev, mode, None)
                occ, occ_keep = base.struct(dev) if base is not None else (None, None)
                rgb = torch.empty((chunk, 3), dtype=torch.float32, device=dev)
                depth = torch.empty((chunk,), dtype=torch.float32, device=dev)
                w = torch.empty((chunk, S), dtype=torch.float32, device=dev)
                z = torch.empty((chunk, S), dtype=torch.float32, device=dev)
                for pose in poses:
                    c2w = _c2w12(pose)
                    for a in range(0, H * W, chunk):
                        b = min(a + chunk, H * W)
                        if occ is not None:
                            L.check(L.lib().nrf_render_camera_occ(h, H, W, float(focal), c2w, a, b, C.byref(opts), C.byref(occ), L.ptr(rgb),
                                                                  L.ptr(depth), L.ptr(w), L.ptr(z), L.stream_ptr()))
                        else:
                            L.check(L.lib().nrf_render_camera(h, H, W, float(focal), c2w, a, b, C.byref(opts), L.ptr(rgb), L.ptr(depth), L.ptr(w),
                                                              L.ptr(z), L.stream_ptr()))
                        L.check(L.lib().nrf_occupancy_mark_camera(H, W, float(focal), c2w, a, b, S, L.ptr(z), L.ptr(w), res, lo, scale, tau,
                                                                  eps if eps is not None else 0.0, hit.data_ptr(),
                                                                  seen.data_ptr() if seen is not None else None, L.stream_ptr()))
                del keep, occ_keep
        finally:
            model.train(was_training)
        return hit, seen

    @classmethod
    def from_views(cls, model, poses, H, W, focal, near, far, n_samples, lo, hi, resolution=128, weight_threshold=0.0, seen_eps=1e-2,
                   unseen="keep", base=None, dilate=1, mma_mode=None, dino=None, lindisp=False, chunk_rays=1 << 16, outside=0):
        """A grid pruned by the weights the views `poses` render (_view_marks):

            (dilate^n(hit) | (~seen if unseen == "keep" else 0)) & (base or all-ones)

        hit: a sample of weight > weight_threshold fell into the cell; seen: a sample fell into it while its ray still had
        transmittance > seen_eps.  unseen="keep" (the default) leaves the cells no marking ray reached -- behind an opaque surface,
        outside every frustum -- to the base grid, "drop" empties them.  With weight_threshold = 0 and dilate = 0 a render of the
        marking views' own rays at the same n_samples is the plain render bit for bit; a larger weight_threshold trades image for
        time: a dropped sample contributed at most weight_threshold of a colour to its pixel.  base: a grid over the same cells (for
        instance from_model's), applied while the views are rendered and to the result.  A V3 grid belongs to ONE source view:
        dino=dict(features=, pose=, focal=, H=, W=) is required."""
        if unseen not in ("keep", "drop"):
            raise ValueError('unseen must be "keep" or "drop"')
        cls._mark_settings(weight_threshold, seen_eps)
        if seen_eps is None and unseen == "keep":
            raise ValueError('unseen="keep" needs a seen_eps')
        res = tuple(int(r) for r in (resolution if hasattr(resolution, "__len__") else (resolution,) * 3))
        probe = cls(torch.zeros((res[0] * res[1] * res[2] // 32,), dtype=torch.int32), res, lo, hi, outside)        # validates res / box
        if base is not None:
            probe._same_cells(base)
        if model.net == L.NRF_NET_V3 and dino is None:
            raise ValueError("a use_dino model's weights depend on the source view: from_views needs dino=dict(features=, pose=, focal=, H=, W=)")
        L.require_gpu()
        if base is not None and base.bits.is_cuda:
            device = base.bits.device
        else:
            p = next(model.parameters())
            device = p.device if p.is_cuda else torch.device("cuda", torch.cuda.current_device())
        probe = probe.to(device)
        hit, seen = probe._view_marks(model, poses, H, W, focal, near, far, n_samples, weight_threshold=weight_threshold,
                                     seen_eps=seen_eps if unseen == "keep" else None, base=base, mma_mode=mma_mode, dino=dino, lindisp=lindisp,
                                     chunk_rays=chunk_rays)
        grid = probe._like(hit)
        if dilate:
            grid = grid.dilate(dilate)
        if unseen == "keep":
            grid = grid | ~probe._like(seen)
        return grid & base if base is not None else grid

    def prune(self, model, poses, H, W, focal, near, far, n_samples, **kw):
        """from_views(..., base=self) on this grid's own box, resolution and `outside`: the grid with the cells emptied that the
        views `poses` show to be empty."""
        return OccupancyGrid.from_views(model, poses, H, W, focal, near, far, n_samples, self.lo, self.hi, resolution=self.res, base=self,
                                        outside=self.outside, **kw)

    # ---- the C struct -----------------------------------------------------------------------------
    def struct(self, device, stats=None):
        """(nrf_occupancy for a launch on `device`, tensors to keep alive).  stats: an int64 device tensor [2] the call adds to."""
        if not self.bits.is_cuda or self.bits.device != torch.device(device):
            self.bits = self.bits.to(device)                          # moved once, then reused
        return L.occupancy(self.bits.data_ptr(), self.res, self.lo, self.scale, self.outside,
                           stats.data_ptr() if stats is not None else None), (self.bits, stats)


def occupancy_arg(occupancy, return_stats, tail_mode, device):
    """What a render call passes for `occupancy=` / `return_stats=`: (nrf_occupancy or None, stats tensor or None, keep-alive)."""
    if occupancy is None:
        if return_stats:
            raise ValueError("return_stats needs occupancy=: the statistics are those of the skipping kernel")
        return None, None, None
    if tail_mode is not None:
        raise ValueError("occupancy cannot be combined with tail_mode: the grid is not part of the tail family")
    stats = torch.zeros((2,), dtype=torch.int64, device=device) if return_stats else None
    st, keep = occupancy.struct(device, stats)
    return st, stats, keep
