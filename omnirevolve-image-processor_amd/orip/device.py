"""Device: one orip_ctx (one GPU, one HIP stream) with numpy-array marshalling around the C ABI."""
from __future__ import annotations

import ctypes as C
from typing import List, Sequence, Tuple

import numpy as np

from . import lib as _l


class OripError(RuntimeError):
    pass


class _Resident:
    def __repr__(self):
        return "RESIDENT"


RESIDENT = _Resident()      # kmeans_fit / kmeans_fit_rgb: fit from the sample set kmeans_samples left in the context


def _p(a: np.ndarray):
    return a.ctypes.data_as(C.c_void_p)


def _mm_paths(off, pts_mm, n):
    """mm paths for the C side: (off pointer, pts pointer, n, the arrays that own the memory); both None = the n fitted paths resident on the device"""
    if off is None and pts_mm is None:
        return None, None, int(n), ()
    o = np.ascontiguousarray(off, np.int64).reshape(-1)
    p = np.ascontiguousarray(pts_mm, np.float64).reshape(-1, 2)
    n = max(len(o) - 1, 0)
    if n and int(o[-1]) != len(p):
        raise ValueError(f"offsets end at {int(o[-1])}, {len(p)} points given")
    return _p(o) if n else None, _p(p) if len(p) else None, n, (o, p)


def _step_paths(off, pts, n):
    """step polylines for the C side, as _mm_paths; both None = the n resident ones (n may still be None: the caller may know it from elsewhere)"""
    if off is None and pts is None:
        return None, None, n, ()
    if off is None or pts is None:
        raise OripError("off and pts: both or neither")
    o = np.ascontiguousarray(off, np.int64).reshape(-1)
    p = np.ascontiguousarray(pts, np.int32).reshape(-1, 2)
    if len(o) < 1 or int(o[-1]) != len(p):
        raise OripError(f"offsets end at {int(o[-1]) if len(o) else None}, {len(p)} points given")
    if len(p) == 0:
        p = np.zeros((1, 2), np.int32)                           # n == 0: a pointer all the same, so that the form stays the explicit one
    return _p(o), _p(p), len(o) - 1, (o, p)


def _groups(group, n):
    """(group int32 [n] or None = all 0, n) of a call that takes one group per path; n: the count _step_paths found, or None when only the groups tell it"""
    g = None
    if group is not None:
        g = np.ascontiguousarray(group, np.int32).reshape(-1)
        n = len(g) if n is None else n
        if len(g) != n:
            raise ValueError(f"{len(g)} groups given for {n} paths")
    if n is None:
        raise ValueError("n: the number of resident step polylines")
    return g, int(n)


def _start_xy(start) -> np.ndarray:
    st = np.asarray(start, np.int64).reshape(-1)
    if len(st) != 2 or (st < 0).any() or (st > 1 << 30).any():
        raise OripError(f"start {tuple(st.tolist())} outside 0..2^30")
    return np.ascontiguousarray(st, np.int32)


class Device:
    def __init__(self, device_id: int = 0):
        self.L = _l.load()
        h = C.c_void_p()
        rc = self.L.orip_create(int(device_id), C.byref(h))
        if rc != 0 or not h:
            raise OripError(f"orip_create(device={device_id}) failed with {rc}: no usable MI355X (there is no CPU fallback)")
        self.h = h
        self.H = self.W = self.K = 0

    def close(self):
        cached = getattr(self, "_comm", None)       # communicator of sharded steps (orip.parallel.comm_of)
        if cached is not None and getattr(self, "h", None):
            self._comm = None
            try:
                cached[1].close()
            except Exception:
                pass
        if getattr(self, "h", None):
            self.L.orip_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _ck(self, rc: int):
        if rc != 0:
            raise OripError((self.L.orip_last_error(self.h) or b"?").decode())

    def sync(self):
        self._ck(self.L.orip_sync(self.h))

    # ---- profiling hooks (bench.py roofline leg)
    def prof_enable(self, on: bool): self._ck(self.L.orip_prof_enable(self.h, int(on)))
    def prof_reset(self): self._ck(self.L.orip_prof_reset(self.h))

    def prof_get(self, kernel: str) -> Tuple[float, int]:
        ms, n = C.c_double(0), C.c_int64(0)
        self._ck(self.L.orip_prof_get(self.h, kernel.encode(), C.byref(ms), C.byref(n)))
        return ms.value, n.value

    # ---- stage 01
    def resize_area(self, img: np.ndarray, new_w: int, new_h: int, as_image: bool = False, fetch: bool = True):
        """cv2.resize(img, (new_w, new_h), interpolation=cv2.INTER_AREA) for shrinking (01:19); as_image leaves the result as the stage-02 image"""
        img = np.ascontiguousarray(img, np.uint8)
        cn = 1 if img.ndim == 2 else img.shape[2]
        out = np.empty((new_h, new_w) if img.ndim == 2 else (new_h, new_w, cn), np.uint8) if fetch else None
        self._ck(self.L.orip_resize_area(self.h, _p(img), img.shape[0], img.shape[1], cn, new_h, new_w, _p(out) if fetch else None, int(as_image)))
        if as_image:
            self.H, self.W = new_h, new_w
        return out

    # ---- stage 02
    def set_image(self, bgr: np.ndarray):
        bgr = np.ascontiguousarray(bgr, np.uint8)
        if bgr.ndim == 2:  # _ensure_bgr (02:25-30)
            bgr = np.ascontiguousarray(np.repeat(bgr[:, :, None], 3, axis=2))
        assert bgr.ndim == 3 and bgr.shape[2] == 3
        self.H, self.W = bgr.shape[:2]
        self._img_ref = bgr  # keep alive until the async copy is consumed
        self._ck(self.L.orip_set_image(self.h, _p(bgr), self.H, self.W))
        self.sync()

    def lab_of(self, idx: np.ndarray | None = None) -> np.ndarray:
        if idx is None:
            out = np.empty((self.H, self.W, 3), np.uint8)
            self._ck(self.L.orip_lab_of(self.h, None, 0, _p(out)))
            return out
        idx = np.ascontiguousarray(idx, np.int64)
        out = np.empty((len(idx), 3), np.uint8)
        self._ck(self.L.orip_lab_of(self.h, _p(idx), len(idx), _p(out)))
        return out

    def _kmeans(self, fit, sample_idx, K: int, attempts, max_iter, eps) -> Tuple[np.ndarray, float]:
        """sample_idx: None = every pixel, RESIDENT = the set of kmeans_samples, else the indices (uploaded by this call)"""
        centers = np.zeros((K, 3), np.float32)
        comp = C.c_double(0)
        if sample_idx is None:
            self._ck(fit(self.h, None, 0, K, attempts, max_iter, eps, _p(centers), C.byref(comp)))
        elif sample_idx is RESIDENT:
            self._ck(fit(self.h, None, -1, K, attempts, max_iter, eps, _p(centers), C.byref(comp)))
        else:
            idx = np.ascontiguousarray(sample_idx, np.int64)
            self._ck(fit(self.h, _p(idx), len(idx), K, attempts, max_iter, eps, _p(centers), C.byref(comp)))
        return centers, comp.value

    def kmeans_fit(self, sample_idx, K: int, attempts=3, max_iter=40, eps=0.5) -> Tuple[np.ndarray, float]:
        return self._kmeans(self.L.orip_kmeans_fit, sample_idx, K, attempts, max_iter, eps)

    def kmeans_samples(self, sample_idx: np.ndarray | None):
        """leave the sample set resident for fits with RESIDENT (None: drop it); it lives until an image of another pixel count is set"""
        self._km_key = None              # whatever kmeans_fit_subsampled left is gone
        if sample_idx is None:
            self._ck(self.L.orip_kmeans_samples(self.h, None, 0))
            return
        idx = np.ascontiguousarray(sample_idx, np.int64)
        self._ck(self.L.orip_kmeans_samples(self.h, _p(idx), len(idx)))

    def kmeans_samples_info(self) -> Tuple[int, int]:
        """(indices, pixel count of the image they were made for) of the resident sample set; (0, 0): none"""
        n, npx = C.c_int64(0), C.c_int64(0)
        self._ck(self.L.orip_kmeans_samples_info(self.h, C.byref(n), C.byref(npx)))
        return n.value, npx.value

    def kmeans_fit_subsampled(self, limit: int, K: int, attempts=3, max_iter=40, eps=0.5, rgb: bool = False) -> Tuple[np.ndarray, float]:
        """The fit of stage 02 on its fixed-seed subsample (orip.stages.subsample_indices: a function of the pixel count and `limit` alone).  The set is built
        and uploaded only when the context does not hold the one of (H * W, limit) already -- decided from what the library reports and from which
        (pixel count, limit) this object uploaded last, never from array contents."""
        from . import stages as S
        fit = self.kmeans_fit_rgb if rgb else self.kmeans_fit
        npx, limit = self.H * self.W, int(limit)
        if npx <= limit:
            return fit(None, K, attempts, max_iter, eps)
        if getattr(self, "_km_key", None) != (npx, limit) or self.kmeans_samples_info() != (limit, npx):
            self.kmeans_samples(S.subsample_indices(npx, limit))
            self._km_key = (npx, limit)
        return fit(RESIDENT, K, attempts, max_iter, eps)

    # ---- process_colors.py
    def kmeans_fit_rgb(self, sample_idx, K: int, attempts=3, max_iter=30, eps=1.0) -> Tuple[np.ndarray, float]:
        """kmeans_palette's cv2.kmeans (process_colors.py:41-45) over the R, G, B bytes of the sampled pixels; float centres in R, G, B order"""
        return self._kmeans(self.L.orip_kmeans_fit_rgb, sample_idx, K, attempts, max_iter, eps)

    def assign_palette(self, palette_rgb: np.ndarray, fetch: bool = True):
        """assign_labels (process_colors.py:69-77): (labels u8 [H,W] or None, pixels per label)"""
        pal = np.ascontiguousarray(palette_rgb, np.uint8).reshape(-1, 3)
        labels = np.empty((self.H, self.W), np.uint8) if fetch else None
        counts = np.zeros(len(pal), np.int64)
        self._ck(self.L.orip_assign_palette(self.h, _p(pal), len(pal), _p(labels) if fetch else None, _p(counts)))
        return labels, counts

    # ---- analyze_colors.py (include/orip.h; csrc/analyze.hip)
    def colors_table(self, ignore_white: bool = True, white_threshold: int = 240, min_kept: int = 100, fetch: bool = True):
        """the exact colour table of the kept pixels (:58-67), left resident: (keys u32 [D] = R<<16|G<<8|B ascending, counts int64 [D], kept pixels,
        used_all: fewer than min_kept pixels passed the filter and every pixel was kept); keys and counts are None without fetch"""
        d, kept, ua = C.c_int64(0), C.c_int64(0), C.c_int32(0)
        self._ck(self.L.orip_colors_table(self.h, int(bool(ignore_white)), int(white_threshold), int(min_kept), C.byref(d), C.byref(kept), C.byref(ua)))
        self._colors_D = int(d.value)
        if not fetch:
            return None, None, int(kept.value), bool(ua.value)
        keys = np.zeros(max(d.value, 1), np.uint32); counts = np.zeros(max(d.value, 1), np.int64)
        self._ck(self.L.orip_colors_fetch(self.h, _p(keys), _p(counts), C.byref(kept)))
        return keys[:d.value], counts[:d.value], int(kept.value), bool(ua.value)

    def colors_hue(self) -> np.ndarray:
        """kept pixels per bucket of _build_hue_histogram (:128-167), int64 [11] in orip.analyze.HUE_KEYS order"""
        out = np.zeros(11, np.int64)
        self._ck(self.L.orip_colors_hue(self.h, _p(out)))
        return out

    def colors_kmeans(self, K: int, n_init: int = 10, max_iter: int = 300, seed: int = 42):
        """weighted k-means over the resident table: (centers float64 [n_init,K,3], n int64 [n_init,K], sums int64 [n_init,K,3], iterations int32 [n_init])"""
        K, n_init = int(K), int(n_init)
        if K < 1 or n_init < 1:
            raise ValueError(f"K={K}, n_init={n_init}")
        cen = np.zeros((n_init, K, 3), np.float64); n = np.zeros((n_init, K), np.int64); sums = np.zeros((n_init, K, 3), np.int64); it = np.zeros(n_init, np.int32)
        self._ck(self.L.orip_colors_kmeans(self.h, K, n_init, int(max_iter), int(seed) & 0xFFFFFFFFFFFFFFFF, _p(cen), _p(n), _p(sums), _p(it)))
        return cen, n, sums, it

    def lab_of_rgb(self, rgb) -> np.ndarray:
        """stage 02's BGR2LAB of R, G, B triples [n,3] -> uint8 [n,3]"""
        a = np.ascontiguousarray(np.asarray(rgb).reshape(-1, 3), np.uint8)
        out = np.zeros((max(len(a), 1), 3), np.uint8)
        self._ck(self.L.orip_lab_of_rgb(self.h, _p(a) if len(a) else None, len(a), _p(out) if len(a) else None))
        return out[:len(a)]

    def extract_layers(self, centers: np.ndarray, open_iters=1, close_iters=1, want_counts=True):
        c = np.ascontiguousarray(centers, np.float32)
        K = len(c)
        cs = np.zeros((K, 3), np.float32)
        counts = np.zeros(K, np.int64)
        self._ck(self.L.orip_extract_layers(self.h, _p(c), K, open_iters, close_iters, _p(cs), _p(counts) if want_counts else None))
        self.K = K
        return cs, counts

    def get_labels(self) -> np.ndarray:
        out = np.empty((self.H, self.W), np.uint8)
        self._ck(self.L.orip_get_labels(self.h, _p(out)))
        return out

    def get_mask(self, layer: int) -> np.ndarray:
        out = np.empty((self.H, self.W), np.uint8)
        self._ck(self.L.orip_get_mask(self.h, layer, _p(out)))
        return out

    def set_masks(self, masks: np.ndarray):
        m = np.ascontiguousarray(masks, np.uint8)
        self.K, self.H, self.W = m.shape
        self._ck(self.L.orip_set_masks(self.h, _p(m), self.K, self.H, self.W))
        self.sync()

    def keep_layers(self, layers: Sequence[int]):
        a = np.ascontiguousarray(np.asarray(list(layers), np.int32))
        self._ck(self.L.orip_keep_layers(self.h, _p(a), len(a)))
        self.K = len(a)

    # ---- stage 03
    def detect_edges(self, morph_k=3, open_iters=1, close_iters=1, gauss_k=3, low=50, high=150):
        self._ck(self.L.orip_detect_edges(self.h, morph_k, open_iters, close_iters, gauss_k, int(low), int(high)))

    def get_edges(self, layer: int) -> np.ndarray:
        out = np.empty((self.H, self.W), np.uint8)
        self._ck(self.L.orip_get_edges(self.h, layer, _p(out)))
        return out

    def set_edges(self, edges: np.ndarray):
        e = np.ascontiguousarray(edges, np.uint8)
        self.K, self.H, self.W = e.shape
        self._ck(self.L.orip_set_edges(self.h, _p(e), self.K, self.H, self.W))
        self.sync()

    # ---- stage 04
    def find_contours(self):
        self._ck(self.L.orip_find_contours(self.h))

    def contours_reserve(self, K: int):
        """hint: K layers of the image just set will be traced (allocates stage 04's memo planes at the start of the step; clears nothing)"""
        self._ck(self.L.orip_contours_reserve(self.h, int(K)))

    def contours_prepare(self):
        self._ck(self.L.orip_contours_prepare(self.h))

    def contours_layer(self, layer: int):
        self._ck(self.L.orip_contours_layer(self.h, layer))

    def get_skeleton(self, layer: int) -> np.ndarray:
        out = np.empty((self.H, self.W), np.uint8)
        self._ck(self.L.orip_get_skeleton(self.h, layer, _p(out)))
        return out

    # ---- slots
    def polys_size(self, slot: int, layer: int) -> Tuple[int, int]:
        n, t = C.c_int64(0), C.c_int64(0)
        self._ck(self.L.orip_polys_size(self.h, slot, layer, C.byref(n), C.byref(t)))
        return n.value, t.value

    def get_polys_flat(self, slot: int, layer: int) -> Tuple[np.ndarray, np.ndarray]:
        n, t = self.polys_size(slot, layer)
        off = np.zeros(n + 1, np.int64)
        pts = np.zeros((max(t, 1), 2), np.int32)
        self._ck(self.L.orip_get_polys(self.h, slot, layer, _p(off), _p(pts)))
        return off, pts[:t]

    def get_polys_offsets(self, slot: int, layer: int) -> np.ndarray:
        """off int64[n + 1] only: a walk-coded list is not expanded for this"""
        n, _ = self.polys_size(slot, layer)
        off = np.zeros(n + 1, np.int64)
        self._ck(self.L.orip_get_polys(self.h, slot, layer, _p(off), None))
        return off

    def get_polys(self, slot: int, layer: int) -> List[np.ndarray]:
        off, pts = self.get_polys_flat(slot, layer)
        return [pts[off[i]:off[i + 1]].reshape(-1, 1, 2) for i in range(len(off) - 1)]

    def set_polys(self, slot: int, layer: int, polys: Sequence[np.ndarray]):
        n = len(polys)
        flat = [np.asarray(p).reshape(-1, 2).astype(np.int32) for p in polys]
        off = np.zeros(n + 1, np.int64)
        for i, p in enumerate(flat):
            off[i + 1] = off[i] + len(p)
        pts = np.ascontiguousarray(np.concatenate(flat, 0) if n else np.zeros((1, 2), np.int32), np.int32)
        self._ck(self.L.orip_set_polys(self.h, slot, layer, n, _p(off), _p(pts)))

    def get_taps(self, which: int, layer: int) -> List[Tuple[int, int]]:
        n = C.c_int64(0)
        self._ck(self.L.orip_taps_size(self.h, which, layer, C.byref(n)))
        a = np.zeros((max(n.value, 1), 2), np.int32)
        self._ck(self.L.orip_get_taps(self.h, which, layer, _p(a)))
        return [(int(x), int(y)) for x, y in a[:n.value]]

    def set_taps(self, which: int, layer: int, taps: Sequence[Tuple[int, int]]):
        a = np.ascontiguousarray(np.asarray(list(taps), np.int32).reshape(-1, 2))
        self._ck(self.L.orip_set_taps(self.h, which, layer, len(a), _p(a) if len(a) else None))

    def set_layer_count(self, K: int):
        self._ck(self.L.orip_set_layer_count(self.h, K))
        self.K = K

    # ---- stages 05 .. 12
    def scale_vectors(self, layer: int, sx, sy, dx, dy):
        self._ck(self.L.orip_scale_vectors(self.h, layer, np.float32(sx), np.float32(sy), np.float32(dx), np.float32(dy)))

    def sort_contours(self, layer: int):
        self._ck(self.L.orip_sort_contours(self.h, layer))

    def dedup_layer(self, layer: int, prm: _l.Params08):
        self._ck(self.L.orip_dedup_layer(self.h, layer, C.byref(prm)))

    def layer_front(self, layer: int, sx, sy, dx, dy, upto: int, prm: _l.Params08 | None):
        """contours_layer -> scale_vectors [-> sort_contours [-> dedup_layer]] (upto 5 / 7 / 8) in one call on the layer's lane"""
        self._ck(self.L.orip_layer_front(self.h, layer, np.float32(sx), np.float32(sy), np.float32(dx), np.float32(dy), int(upto), C.byref(prm) if prm is not None else None))

    def dedup_cross(self, order: Sequence[int], prm: _l.Params10):
        o = np.ascontiguousarray(np.asarray(list(order), np.int32))
        self._ck(self.L.orip_dedup_cross(self.h, _p(o), len(o), C.byref(prm)))

    def dedup_cross_begin(self, prm: _l.Params10):
        self._ck(self.L.orip_dedup_cross_begin(self.h, C.byref(prm)))

    def dedup_cross_layer(self, layer: int, src_layer: int | None = None, defer_reorder: bool = False):
        """defer_reorder: leave the travel reorder of the layer's lines (10:253) to plot_order(layer) -- resident pipelines only"""
        src = layer if src_layer is None else src_layer
        if defer_reorder:
            self._ck(self.L.orip_dedup_cross_layer_deferred(self.h, src, layer))
        else:
            self._ck(self.L.orip_dedup_cross_layer_from(self.h, src, layer))

    # ---- 13_build_stream: direction codes of all moves of a plot
    def stream_codes(self, moves: np.ndarray, fetch_codes: bool = True) -> Tuple[np.ndarray, np.ndarray | None]:
        """moves int32 [n,4] (x0, y0, x1, y1) -> (off int64 [n+1], codes uint8 [total]); without the fetch the codes stay on the device for
        stream_pack and (off, None) comes back"""
        m = np.ascontiguousarray(moves, np.int32).reshape(-1, 4)
        total = C.c_int64(0)
        self._ck(self.L.orip_stream_codes(self.h, _p(m) if len(m) else None, len(m), C.byref(total)))
        off = np.zeros(len(m) + 1, np.int64)
        codes = np.zeros(max(total.value, 1), np.uint8) if fetch_codes else None
        self._ck(self.L.orip_stream_codes_fetch(self.h, _p(off), _p(codes) if fetch_codes else None))
        return off, codes[:total.value] if fetch_codes else None

    def stream_preview(self, data, W: int, H: int, rw: int, rh: int, flags: int, palette, tap_radius: int) -> Tuple[np.ndarray, dict]:
        """decode + replay + draw a plotter stream (include/orip.h: orip_stream_preview) -> (rgb uint8 [rh, rw, 3], statistics dict);
        rw x rh is the surface as drawn (orip.stream_preview.render_size applies the previewer's clamp)"""
        from .stream_preview import STAT_FIELDS
        d = np.ascontiguousarray(np.frombuffer(bytes(data), np.uint8) if isinstance(data, (bytes, bytearray)) else data, np.uint8).reshape(-1)
        pal = np.ascontiguousarray(np.asarray(palette, np.int64).reshape(4, 3), np.uint8)
        st = np.zeros(len(STAT_FIELDS), np.int64)
        self._ck(self.L.orip_stream_preview(self.h, _p(d) if len(d) else None, len(d), int(W), int(H), int(rw), int(rh), int(flags), _p(pal), int(tap_radius), _p(st)))
        rgb = np.zeros((int(rh), int(rw), 3), np.uint8)
        self._ck(self.L.orip_stream_preview_fetch(self.h, _p(rgb)))
        return rgb, {k: int(v) for k, v in zip(STAT_FIELDS, st)}

    # ---- gcode2stream: paths to steps, nearest-neighbour order, stream bytes (include/orip.h; csrc/gcode.hip)
    def gcode_to_steps(self, off: np.ndarray | None, pts_mm: np.ndarray | None, map: dict, fetch_points: bool = True, n: int | None = None) -> Tuple[np.ndarray, np.ndarray]:
        """paths in mm (off int64 [n + 1], pts float64 [total, 2]) -> step polylines (off int64, pts int32 [total', 2]), also left resident;
        off = pts_mm = None: the n fitted paths svg_flatten / svg_fit left on the device; map: the fields of orip_gcode_map"""
        po, pp, n, _keep = _mm_paths(off, pts_mm, n)
        m = _l.GcodeMap(**{k: map[k] for k, _ in _l.GcodeMap._fields_})
        n_out, tot = C.c_int64(0), C.c_int64(0)
        self._ck(self.L.orip_gcode_to_steps(self.h, po, pp, n, C.byref(m), C.byref(n_out), C.byref(tot)))
        return self.gcode_steps_fetch(n_out.value, tot.value, fetch_points)

    def gcode_to_steps_clip(self, off: np.ndarray | None, pts_mm: np.ndarray | None, map: dict, rect, n: int | None = None) -> Tuple[np.ndarray, np.ndarray, dict]:
        """--clip (include/orip.h: orip_gcode_to_steps_clip): gcode_to_steps with the strokes cut at rect = (x0, y0, x1, y1) in steps instead of clamped to
        the sheet; the strokes are left resident as gcode_to_steps leaves its polylines.  off = pts_mm = None: the n fitted paths on the device.
        -> (off int64, pts int32 [total', 2], {"segments", "inside", "cut", "outside", "paths_out", "points_out"})"""
        po, pp, n, _keep = _mm_paths(off, pts_mm, n)
        r = np.asarray(rect, np.int64).reshape(-1)
        if len(r) != 4 or (np.abs(r) > 1 << 30).any():
            raise OripError(f"clip rectangle {tuple(r.tolist())}: four step coordinates")
        r = np.ascontiguousarray(r, np.int32)
        m = _l.GcodeMap(**{k: map[k] for k, _ in _l.GcodeMap._fields_})
        n_out, tot = C.c_int64(0), C.c_int64(0)
        st = np.zeros(len(_l.CLIP_STATS), np.int64)
        self._ck(self.L.orip_gcode_to_steps_clip(self.h, po, pp, n, C.byref(m), _p(r), C.byref(n_out), C.byref(tot), _p(st)))
        off_s, pts_s = self.gcode_steps_fetch(n_out.value, tot.value)
        return off_s, pts_s, {k: int(v) for k, v in zip(_l.CLIP_STATS, st)}

    # ---- svg2stream: flatten, bounding box, fit (include/orip.h; csrc/svg.hip)
    def svg_flatten(self, table, tol: float) -> int:
        """segments of an orip.svg.SegmentTable (mats: its raw matrices) -> resident polylines in raw units; returns the number of points"""
        kind = np.ascontiguousarray(table.kind, np.int32).reshape(-1); ctrl = np.ascontiguousarray(table.ctrl, np.float64).reshape(-1, 4, 2)
        mi = np.ascontiguousarray(table.mat, np.int32).reshape(-1); sub = np.ascontiguousarray(table.sub_off, np.int64).reshape(-1)
        mats = np.ascontiguousarray(table.raw_mats(), np.float64).reshape(-1, 6)
        if not (len(kind) == len(ctrl) == len(mi)) or len(sub) < 1:
            raise ValueError("segment table: kind, ctrl and mat must have one entry per segment, sub_off at least one")
        ns, nsub = len(kind), len(sub) - 1
        self._svg_n = 0
        total = C.c_int64(0)
        self._ck(self.L.orip_svg_flatten(self.h, _p(kind) if ns else None, _p(ctrl) if ns else None, _p(mi) if ns else None, ns, _p(sub) if ns else None, nsub,
                                         _p(mats) if len(mats) else None, len(mats), float(tol), C.byref(total)))
        self._svg_n = nsub
        return int(total.value)

    def gcode_flatten(self, table, tol: float) -> Tuple[int, dict]:
        """--arcs (include/orip.h: orip_gcode_flatten): the lines and arcs of an orip.gcode.ArcTable (kind, seg, sub_off) -> resident polylines in mm, as
        svg_flatten leaves its own: svg_paths fetches them, gcode_to_steps / gcode_to_steps_clip(None, None, ..., n=) convert them.
        -> (the number of points, {"arcs", "pieces", "full_circles"})"""
        kind = np.ascontiguousarray(table[0], np.int32).reshape(-1); seg = np.ascontiguousarray(table[1], np.float64).reshape(-1, 6)
        sub = np.ascontiguousarray(table[2], np.int64).reshape(-1)
        if len(kind) != len(seg) or len(sub) < 1:
            raise ValueError("arc table: kind and seg must have one entry per segment, sub_off at least one")
        ns, nsub = len(kind), len(sub) - 1
        self._svg_n = 0
        total = C.c_int64(0)
        st = np.zeros(len(_l.ARC_STATS), np.int64)
        self._ck(self.L.orip_gcode_flatten(self.h, _p(kind) if ns else None, _p(seg) if ns else None, ns, _p(sub) if ns else None, nsub, float(tol), C.byref(total), _p(st)))
        self._svg_n = nsub
        return int(total.value), {k: int(v) for k, v in zip(_l.ARC_STATS, st)}

    def svg_paths(self, n: int | None = None, with_points: bool = True):
        """the resident paths, flattened or fitted: (off int64 [n + 1], pts float64 [total, 2], or None without the points)"""
        n = self._svg_n if n is None else int(n)
        off = np.zeros(n + 1, np.int64)
        self._ck(self.L.orip_svg_paths_fetch(self.h, _p(off), None))
        if not with_points:
            return off, None
        pts = np.zeros((max(int(off[-1]), 1), 2), np.float64)
        self._ck(self.L.orip_svg_paths_fetch(self.h, _p(off), _p(pts)))
        return off, pts[:int(off[-1])]

    def svg_bbox(self) -> Tuple[float, float, float, float]:
        """(min x, min y, max x, max y) of the resident points"""
        box = np.zeros(4, np.float64)
        self._ck(self.L.orip_svg_bbox(self.h, _p(box)))
        return tuple(float(v) for v in box)

    def svg_fit(self, sx: float, sy: float, ox: float, oy: float) -> None:
        """v * s + o per axis, rounded to four decimals as float(f"{v:.4f}") rounds, in place on the resident paths"""
        self._ck(self.L.orip_svg_fit(self.h, float(sx), float(sy), float(ox), float(oy)))

    def _svg_hatch(self, call, names, fill_group, steps_per_mm, spacing, inset, *rest) -> dict:
        """either hatch call: the group array, the stats array, the resident count moved on by the appended segments -> the counts by name"""
        g = np.ascontiguousarray(fill_group, np.int32).reshape(-1)
        st = np.zeros(len(names), np.int64)
        self._ck(call(self.h, _p(g) if len(g) else None, len(g), float(steps_per_mm), int(spacing), int(inset), *rest, _p(st)))
        self._svg_n = len(g) + int(st[names.index("segments")])
        return {k: int(v) for k, v in zip(names, st)}

    def svg_hatch(self, fill_group, steps_per_mm: float, spacing: int, inset: int, flags: int) -> dict:
        """hatch lines of the fitted resident paths, appended to them as 2-point paths (include/orip.h: orip_svg_hatch; flags: orip.lib.HATCH_*);
        fill_group int32 per resident subpath, -1 or its group -> {"groups", "lines", "crossings", "segments"}"""
        return self._svg_hatch(self.L.orip_svg_hatch, _l.HATCH_STATS, fill_group, steps_per_mm, spacing, inset, int(flags))

    def svg_hatch_angle(self, fill_group, steps_per_mm: float, spacing: int, inset: int, u, flags: int) -> dict:
        """hatch lines along the integer direction u = (ux, uy), exact on the step grid, appended as svg_hatch appends its own (include/orip.h:
        orip_svg_hatch_angle) -> {"groups", "lines", "crossings", "segments", "collapsed"}"""
        ux, uy = (int(v) for v in u)
        if max(abs(ux), abs(uy)) >= 2 ** 31:
            raise ValueError("the hatch direction must fit 32 bits")
        return self._svg_hatch(self.L.orip_svg_hatch_angle, _l.HATCH_ANGLE_STATS, fill_group, steps_per_mm, spacing, inset, ux, uy, int(flags))

    def gcode_order(self, ends: np.ndarray | None, n: int | None = None) -> np.ndarray:
        """order of the paths (first x, first y, last x, last y) int32 [n, 4]; ends None: the n resident step polylines of gcode_to_steps"""
        if ends is not None:
            e = np.ascontiguousarray(ends, np.int32).reshape(-1, 4)
            n = len(e)
        order = np.zeros(max(int(n), 1), np.int32)
        self._ck(self.L.orip_gcode_order(self.h, _p(e) if ends is not None and n else None, int(n), _p(order)))
        return order[:int(n)]

    def gcode_order_pens(self, ends: np.ndarray | None, group, n_groups: int, reverse: bool = False, start=(0, 0), n: int | None = None) -> Tuple[np.ndarray, np.ndarray]:
        """group after group from `start`, inside a group the nearest remaining end (include/orip.h: orip_gcode_order_pens) -> (order int32 [n], rev bool [n]);
        ends int32 [n, 4] or None for the n resident step polylines, group int32 [n] in 0 .. n_groups - 1, reverse: strokes may be drawn backwards"""
        g = np.ascontiguousarray(group, np.int32).reshape(-1)
        if ends is not None:
            e = np.ascontiguousarray(ends, np.int32).reshape(-1, 4)
            n = len(e)
        n = len(g) if n is None else int(n)
        if len(g) != n:
            raise ValueError(f"{len(g)} groups given for {n} paths")
        st = _start_xy(start)
        order = np.zeros(max(n, 1), np.int32); rev = np.zeros(max(n, 1), np.uint8)
        self._ck(self.L.orip_gcode_order_pens(self.h, _p(e) if ends is not None and n else None, _p(g) if n else None, n, int(n_groups), _l.ORDER_REVERSE if reverse else 0,
                                              _p(st), _p(order), _p(rev)))
        return order[:n], rev[:n].astype(bool)

    def gcode_improve(self, ends: np.ndarray | None, group, n_groups: int, order, rev, reverse: bool = False, start=(0, 0), max_rounds: int | None = None,
                      n: int | None = None):
        """--improve-order (include/orip.h: orip_gcode_improve): 2-opt and or-opt on the drawing sequence (order int [n], rev bool [n]) of the paths
        ends int32 [n, 4] (None: the n resident step polylines), group after group from `start`; max_rounds None = 2 m + 64 rounds for a group of m strokes.
        -> (order int32 [n], rev bool [n], {"travel_before", "travel_after", "rounds", "converged_groups", "skipped_groups"})"""
        g = np.ascontiguousarray(group, np.int32).reshape(-1)
        if ends is not None:
            e = np.ascontiguousarray(ends, np.int32).reshape(-1, 4)
            n = len(e)
        n = len(g) if n is None else int(n)
        o = np.array(order, np.int32).reshape(-1)                # copies: the call rewrites them in place
        r = np.array(rev, np.uint8).reshape(-1)
        if len(g) != n or len(o) != n or len(r) != n:
            raise ValueError(f"{len(g)} groups, {len(o)} positions and {len(r)} directions given for {n} paths")
        st = _start_xy(start)
        if max_rounds is not None and not (-(1 << 63) <= int(max_rounds) < (1 << 63)):
            raise OripError(f"{max_rounds} rounds")
        if n == 0:
            o = np.zeros(1, np.int32); r = np.zeros(1, np.uint8)
        stats = np.zeros(5, np.int64)
        self._ck(self.L.orip_gcode_improve(self.h, _p(e) if ends is not None and n else None, _p(g) if n else None, n, int(n_groups), _l.ORDER_REVERSE if reverse else 0,
                                           _p(st), _l.IMPROVE_ROUNDS_AUTO if max_rounds is None else int(max_rounds), _p(o), _p(r), _p(stats)))
        return o[:n], r[:n].astype(bool), {k: int(v) for k, v in zip(("travel_before", "travel_after", "rounds", "converged_groups", "skipped_groups"), stats)}

    def gcode_seam(self, off, pts, order, rev, start=(0, 0), n: int | None = None):
        """--loop-start (include/orip.h: orip_gcode_seam): where every closed stroke of the drawing sequence (order int [n], rev bool [n], either None =
        identity / no reversal) is entered and left, for the least pen-up travel from `start`; the step polylines (off int64 [n + 1], pts int32 [total, 2])
        or, both None, the n resident ones, which are read and not changed.
        -> (seam int32 [n]: by sequence position, the stored ring vertex a closed stroke starts and ends at, 0 for an open one,
            {"closed", "moved", "travel_before", "travel_after"})"""
        po, pp, n, _keep = _step_paths(off, pts, n)
        o = None if order is None else np.ascontiguousarray(order, np.int32).reshape(-1)
        r = None if rev is None else np.ascontiguousarray(rev, np.uint8).reshape(-1)
        if n is None:
            n = len(o) if o is not None else len(r) if r is not None else None
        if n is None:
            raise ValueError("n: the number of resident step polylines")
        n = int(n)
        if (o is not None and len(o) != n) or (r is not None and len(r) != n):
            raise ValueError(f"{None if o is None else len(o)} positions and {None if r is None else len(r)} directions given for {n} paths")
        st = _start_xy(start)
        seam = np.zeros(max(n, 1), np.int32)
        stats = np.zeros(4, np.int64)
        self._ck(self.L.orip_gcode_seam(self.h, po, pp, n, _p(o) if o is not None and n else None, _p(r) if r is not None and n else None, _p(st), _p(seam), _p(stats)))
        return seam[:n], {k: int(v) for k, v in zip(_l.SEAM_STATS, stats)}

    def gcode_order_rings(self, off, pts, group, n_groups: int, reverse: bool = False, start=(0, 0), n: int | None = None):
        """--ring-entry (include/orip.h: orip_gcode_order_rings): the greedy walk of gcode_order_pens in which a closed stroke is entered at its nearest ring
        vertex; the step polylines (off int64 [n + 1], pts int32 [total, 2]; strokes of one point are legal) or, both None, the n resident ones, which are
        read and not changed; group int32 [n] or None (all 0).
        -> (order int32 [n], rev bool [n], seam int32 [n]: by sequence position, the stored ring vertex a closed stroke is entered at, 0 for an open one,
            {"closed", "moved", "candidates", "travel"})"""
        po, pp, n, _keep = _step_paths(off, pts, n)
        g, n = _groups(group, n)
        st = _start_xy(start)
        order = np.zeros(max(n, 1), np.int32); rev = np.zeros(max(n, 1), np.uint8); seam = np.zeros(max(n, 1), np.int32)
        stats = np.zeros(4, np.int64)
        self._ck(self.L.orip_gcode_order_rings(self.h, po, pp, _p(g) if g is not None and n else None, n, int(n_groups), _l.ORDER_REVERSE if reverse else 0,
                                               _p(st), _p(order), _p(rev), _p(seam), _p(stats)))
        return order[:n], rev[:n].astype(bool), seam[:n], {k: int(v) for k, v in zip(_l.RING_ENTRY_STATS, stats)}

    def gcode_merge(self, off, pts, group, n_groups: int, reverse: bool = False, n: int | None = None):
        """--merge-paths (include/orip.h: orip_gcode_merge): step polylines (off int64 [n + 1], pts int32 [total, 2]; both None = the n resident ones) that
        meet end to end inside a group become one stroke, and the merged polylines become the resident ones.  group int32 [n] or None (all 0).
        -> (off int64, pts int32 [total', 2], member_off int64 [paths_out + 1], member int32 [n], rev bool [n], {"paths_out", "points_out", "joins", "cycles"})"""
        po, pp, n, _keep = _step_paths(off, pts, n)
        g, n = _groups(group, n)
        st = np.zeros(4, np.int64)
        self._ck(self.L.orip_gcode_merge(self.h, po, pp, _p(g) if g is not None and n else None, n, int(n_groups),
                                         _l.MERGE_REVERSE if reverse else 0, _p(st)))
        paths, total = int(st[0]), int(st[1])
        moff = np.zeros(paths + 1, np.int64); member = np.zeros(max(n, 1), np.int32); rev = np.zeros(max(n, 1), np.uint8)
        self._ck(self.L.orip_gcode_merge_fetch(self.h, _p(moff), _p(member), _p(rev)))
        off_s, pts_s = self.gcode_steps_fetch(paths, total)
        return off_s, pts_s, moff, member[:n], rev[:n].astype(bool), {k: int(v) for k, v in zip(("paths_out", "points_out", "joins", "cycles"), st)}

    def gcode_simplify(self, off, pts, tol4: int, n: int | None = None):
        """--simplify-mm (include/orip.h: orip_gcode_simplify): Ramer-Douglas-Peucker on the step polylines (off int64 [n + 1], pts int32 [total, 2]; both
        None = the n resident ones) with the tolerance tol4 in quarter steps, and the simplified polylines become the resident ones.
        -> (off int64, pts int32 [total', 2], kept int64 [total']: the input index of every output point, {"paths", "points_in", "points_out", "rounds"})"""
        po, pp, n, _keep = _step_paths(off, pts, n)
        if n is None:
            raise ValueError("n: the number of resident step polylines")
        if not (-(1 << 31) <= int(tol4) < (1 << 31)):
            raise OripError(f"tolerance {tol4} quarter steps")
        n = int(n)
        st = np.zeros(4, np.int64)
        self._ck(self.L.orip_gcode_simplify(self.h, po, pp, n, int(tol4), _p(st)))
        total = int(st[2])
        kept = np.zeros(max(total, 1), np.int64)
        self._ck(self.L.orip_gcode_simplify_fetch(self.h, _p(kept)))
        off_s, pts_s = self.gcode_steps_fetch(n, total)
        return off_s, pts_s, kept[:total], {k: int(v) for k, v in zip(("paths", "points_in", "points_out", "rounds"), st)}

    def gcode_dedup(self, off, pts, group, n_groups: int, n: int | None = None):
        """--dedup (include/orip.h: orip_gcode_dedup): of the collinear segments of one group that lie over each other on the step polylines (off int64 [n + 1],
        pts int32 [total, 2]; both None = the n resident ones) only the first drawn copy stays, and what is left becomes the resident polylines.  group
        int32 [n] or None (all 0).
        -> (off int64, pts int32 [total', 2], origin int32 [paths_out]: the input stroke of every output stroke, {lib.DEDUP_STATS})"""
        po, pp, n, _keep = _step_paths(off, pts, n)
        g, n = _groups(group, n)
        st = np.zeros(9, np.int64)
        self._ck(self.L.orip_gcode_dedup(self.h, po, pp, _p(g) if g is not None and n else None, n, int(n_groups), _p(st)))
        return self._cut_result(st, _l.DEDUP_STATS, self.L.orip_gcode_dedup_fetch)

    def _cut_result(self, st, names, fetch):
        """what a cutting pass (dedup, occlusion, dash) left: its stats st under `names`, its origin through `fetch`, the resident polylines
        -> (off int64, pts int32 [total', 2], origin int32 [paths_out], {names})"""
        paths, total = int(st[names.index("paths_out")]), int(st[names.index("points_out")])
        origin = np.zeros(max(paths, 1), np.int32)
        self._ck(fetch(self.h, _p(origin)))
        off_s, pts_s = self.gcode_steps_fetch(paths, total)
        return off_s, pts_s, origin[:paths], {k: int(v) for k, v in zip(names, st)}

    def gcode_occlude(self, off, pts, level, ring_off, ring_pts, ring_level, n: int | None = None):
        """--occlude (include/orip.h: orip_gcode_occlude): of the step polylines (off int64 [n + 1], pts int32 [total, 2]; both None = the n resident ones)
        with level int32 [n] only what no shape of a higher level hides stays, and that becomes the resident polylines.  The shapes are the rings ring_off
        int64 [m + 1], ring_pts int32 [R, 2] (steps, -2^30 .. 2^30) with ring_level int32 [m], non-decreasing; the rings of one level are one shape.
        -> (off int64, pts int32 [total', 2], origin int32 [paths_out]: the input stroke of every output stroke, {lib.OCCLUDE_STATS})"""
        po, pp, n, _keep = _step_paths(off, pts, n)
        lv = np.ascontiguousarray(level, np.int32).reshape(-1)
        n = len(lv) if n is None else int(n)
        if len(lv) != n:
            raise ValueError(f"{len(lv)} levels given for {n} paths")
        ro = np.ascontiguousarray(ring_off, np.int64).reshape(-1)
        rp = np.ascontiguousarray(ring_pts, np.int32).reshape(-1, 2)
        rl = np.ascontiguousarray(ring_level, np.int32).reshape(-1)
        m = len(rl)
        if len(ro) != m + 1 or (m and len(rp) < int(ro[-1])):
            raise ValueError(f"{len(ro)} ring offsets and {len(rp)} ring points given for {m} rings")
        st = np.zeros(10, np.int64)
        self._ck(self.L.orip_gcode_occlude(self.h, po, pp, _p(lv) if n else None, n, _p(ro) if m else None, _p(rp) if m and len(rp) else None, _p(rl) if m else None, m, _p(st)))
        return self._cut_result(st, _l.OCCLUDE_STATS, self.L.orip_gcode_occlude_fetch)

    def svg_occlude(self, level, ring_sub, ring_level, map: dict, clamp: bool, n: int | None = None):
        """--occlude on the resident step polylines (include/orip.h: orip_svg_occlude): ring r is the resident fitted path ring_sub[r], converted on the
        device as the conversion converts (map: the conversion's; clamp: to the sheet, as gcode_to_steps, or not, as gcode_to_steps_clip).
        -> (off, pts, origin, stats) as gcode_occlude"""
        lv = np.ascontiguousarray(level, np.int32).reshape(-1)
        n = len(lv) if n is None else int(n)
        if len(lv) != n:
            raise ValueError(f"{len(lv)} levels given for {n} paths")
        rs = np.ascontiguousarray(ring_sub, np.int32).reshape(-1)
        rl = np.ascontiguousarray(ring_level, np.int32).reshape(-1)
        if len(rs) != len(rl):
            raise ValueError(f"{len(rs)} rings and {len(rl)} ring levels")
        m = len(rl)
        gm = _l.GcodeMap(**{k: map[k] for k, _ in _l.GcodeMap._fields_})
        st = np.zeros(10, np.int64)
        self._ck(self.L.orip_svg_occlude(self.h, _p(lv) if n else None, n, _p(rs) if m else None, _p(rl) if m else None, m, C.byref(gm), _l.OCCLUDE_CLAMP if clamp else 0, _p(st)))
        return self._cut_result(st, _l.OCCLUDE_STATS, self.L.orip_gcode_occlude_fetch)

    def _link_result(self, st, n):
        """what the hatch link left: its stats, member_off / member through the fetch, the resident polylines"""
        d = {k: int(v) for k, v in zip(_l.HATCH_LINK_STATS, st)}
        moff = np.zeros(d["paths_out"] + 1, np.int64); member = np.zeros(max(n, 1), np.int32)
        self._ck(self.L.orip_gcode_hatch_link_fetch(self.h, _p(moff), _p(member)))
        off_s, pts_s = self.gcode_steps_fetch(d["paths_out"], d["points_out"])
        return off_s, pts_s, moff, member[:n], d

    def gcode_hatch_link(self, off, pts, cls, ring_off, ring_pts, ring_group, reach: int, n: int | None = None):
        """--hatch-connect (include/orip.h: orip_gcode_hatch_link): of the step polylines (off int64 [n + 1], pts int32 [total, 2]; both None = the n resident
        ones) the 2-point strokes with cls[k] = 2 g + f >= 0 are joined into zigzags by links of at most `reach` steps that lie inside shape g, and the result
        becomes the resident polylines.  The shapes are the rings ring_off int64 [m + 1], ring_pts int32 [R, 2] (steps, -2^30 .. 2^30) with ring_group int32
        [m], non-decreasing; the rings of one group are one shape.
        -> (off int64, pts int32 [total', 2], member_off int64 [paths_out + 1], member int32 [n], {lib.HATCH_LINK_STATS})"""
        po, pp, n, _keep = _step_paths(off, pts, n)
        cl = np.ascontiguousarray(cls, np.int32).reshape(-1)
        n = len(cl) if n is None else int(n)
        if len(cl) != n:
            raise ValueError(f"{len(cl)} classes given for {n} paths")
        ro = np.ascontiguousarray(ring_off, np.int64).reshape(-1)
        rp = np.ascontiguousarray(ring_pts, np.int32).reshape(-1, 2)
        rg = np.ascontiguousarray(ring_group, np.int32).reshape(-1)
        m = len(rg)
        if len(ro) != m + 1 or (m and len(rp) < int(ro[-1])):
            raise ValueError(f"{len(ro)} ring offsets and {len(rp)} ring points given for {m} rings")
        st = np.zeros(8, np.int64)
        self._ck(self.L.orip_gcode_hatch_link(self.h, po, pp, _p(cl) if n else None, n, _p(ro) if m else None, _p(rp) if m and len(rp) else None, _p(rg) if m else None, m,
                                              int(reach), _p(st)))
        return self._link_result(st, n)

    def svg_hatch_link(self, cls, ring_sub, ring_group, map: dict, clamp: bool, reach: int, n: int | None = None):
        """--hatch-connect on the resident step polylines (include/orip.h: orip_svg_hatch_link): ring r is the resident fitted path ring_sub[r], converted on
        the device as the conversion converts (map: the conversion's; clamp: to the sheet, as gcode_to_steps, or not, as gcode_to_steps_clip).
        -> (off, pts, member_off, member, stats) as gcode_hatch_link"""
        cl = np.ascontiguousarray(cls, np.int32).reshape(-1)
        n = len(cl) if n is None else int(n)
        if len(cl) != n:
            raise ValueError(f"{len(cl)} classes given for {n} paths")
        rs = np.ascontiguousarray(ring_sub, np.int32).reshape(-1)
        rg = np.ascontiguousarray(ring_group, np.int32).reshape(-1)
        if len(rs) != len(rg):
            raise ValueError(f"{len(rs)} rings and {len(rg)} ring groups")
        m = len(rg)
        gm = _l.GcodeMap(**{k: map[k] for k, _ in _l.GcodeMap._fields_})
        st = np.zeros(8, np.int64)
        self._ck(self.L.orip_svg_hatch_link(self.h, _p(cl) if n else None, n, _p(rs) if m else None, _p(rg) if m else None, m, C.byref(gm),
                                            _l.HATCH_LINK_CLAMP if clamp else 0, int(reach), _p(st)))
        return self._link_result(st, n)

    def _stipple_result(self, st):
        """what the stipple left: its stats, the dot list through the fetch"""
        d = {k: int(v) for k, v in zip(_l.STIPPLE_STATS, st)}
        xy = np.zeros((max(d["dots"], 1), 2), np.int32); grp = np.zeros(max(d["dots"], 1), np.int32)
        self._ck(self.L.orip_gcode_stipple_fetch(self.h, _p(xy), _p(grp)))
        return xy[:d["dots"]], grp[:d["dots"]], d

    def gcode_stipple(self, ring_off, ring_pts, ring_group, lattice, inset: int, rect, flags: int):
        """--stipple-mm (include/orip.h: orip_gcode_stipple): the dots of the shapes given as rings ring_off int64 [m + 1], ring_pts int32 [R, 2] (steps,
        -2^30 .. 2^30) with ring_group int32 [m], non-decreasing (the rings of one group are one shape), on the lattice (pitch, row, shift), at least
        `inset` from their shape's outline, inside rect (x0, y0, x1, y1); flags: lib.STIPPLE_SERPENTINE | lib.STIPPLE_OCCLUDE.  Nothing resident changes.
        -> (xy int32 [dots, 2], group int32 [dots], {lib.STIPPLE_STATS})"""
        ro = np.ascontiguousarray(ring_off, np.int64).reshape(-1)
        rp = np.ascontiguousarray(ring_pts, np.int32).reshape(-1, 2)
        rg = np.ascontiguousarray(ring_group, np.int32).reshape(-1)
        m = len(rg)
        if len(ro) != m + 1 or (m and len(rp) < int(ro[-1])):
            raise ValueError(f"{len(ro)} ring offsets and {len(rp)} ring points given for {m} rings")
        p, q, s = (int(v) for v in lattice)
        rc = np.ascontiguousarray(rect, np.int32).reshape(4)
        st = np.zeros(7, np.int64)
        self._ck(self.L.orip_gcode_stipple(self.h, _p(ro) if m else None, _p(rp) if m and len(rp) else None, _p(rg) if m else None, m, p, q, s, int(inset), _p(rc), int(flags), _p(st)))
        return self._stipple_result(st)

    def svg_stipple(self, ring_sub, ring_group, map: dict, clamp: bool, lattice, inset: int, rect, flags: int):
        """--stipple-mm on the resident fitted paths (include/orip.h: orip_svg_stipple): ring r is the resident fitted path ring_sub[r], converted on the
        device as the conversion converts (map: the conversion's; clamp: to the sheet, as gcode_to_steps, or not, as gcode_to_steps_clip).
        -> (xy, group, stats) as gcode_stipple"""
        rs = np.ascontiguousarray(ring_sub, np.int32).reshape(-1)
        rg = np.ascontiguousarray(ring_group, np.int32).reshape(-1)
        if len(rs) != len(rg):
            raise ValueError(f"{len(rs)} rings and {len(rg)} ring groups")
        m = len(rg)
        gm = _l.GcodeMap(**{k: map[k] for k, _ in _l.GcodeMap._fields_})
        p, q, s = (int(v) for v in lattice)
        rc = np.ascontiguousarray(rect, np.int32).reshape(4)
        st = np.zeros(7, np.int64)
        self._ck(self.L.orip_svg_stipple(self.h, _p(rs) if m else None, _p(rg) if m else None, m, C.byref(gm), p, q, s, int(inset), _p(rc),
                                         int(flags) | (_l.STIPPLE_CLAMP if clamp else 0), _p(st)))
        return self._stipple_result(st)

    def fill_mask(self, mask, W: int, H: int, place, u, spacing: int, inset: int, min_len: int, flags: int, layer: int = 0):
        """fill_layers (include/orip.h: orip_fill_mask): the hatch segments of a colour mask u8 [h, w] (nonzero = set; None: the resident mask of `layer`,
        which is only read) on the canvas W x H, the mask placed by place = (num, den, dx, dy), along the direction u = (ux, uy) every `spacing` pixels,
        `inset` pixels inside every run, runs of `min_len` pixels or more; flags: lib.FILL_SERPENTINE | lib.FILL_ALONG | lib.FILL_ACROSS.  Nothing resident
        changes.  -> (seg int32 [segments, 4] = x0 y0 x1 y1 in canvas pixels, in drawing order, {lib.FILL_STATS})"""
        m = None
        if mask is not None:
            m = np.ascontiguousarray(mask, np.uint8)
            if m.ndim != 2:
                raise ValueError(f"mask of shape {m.shape}: [h, w]")
        h, w = (self.H, self.W) if m is None else m.shape
        scal = [int(v) for v in (layer, h, w, W, H, *place, *u, spacing, inset, min_len, flags)]
        if len(scal) != 15:
            raise ValueError("place = (num, den, dx, dy) and u = (ux, uy)")
        if any(abs(v) >= 1 << 31 for v in scal):
            raise OripError(f"orip_fill_mask: an argument does not fit 32 bits: {scal}")
        st = np.zeros(len(_l.FILL_STATS), np.int64)
        self._ck(self.L.orip_fill_mask(self.h, None if m is None else _p(m), *scal, _p(st)))
        d = {k: int(v) for k, v in zip(_l.FILL_STATS, st)}
        seg = np.zeros((max(d["segments"], 1), 4), np.int32)
        self._ck(self.L.orip_fill_fetch(self.h, _p(seg)))
        return seg[:d["segments"]], d

    def fill_link(self, mask, place, reach: int, layer: int = 0):
        """fill connect (include/orip.h: orip_fill_link): the segments of the last fill_mask of this device drawn as zigzags, a link from the end of a
        segment to the start of one on the next line of its family, at most `reach` pixels long, every pixel of it ink of the mask u8 [h, w] (None: the
        resident mask of `layer`) placed by place = (num, den, dx, dy): what the fill was given.  The segment list stays as it is.
        -> (off int64 [paths_out + 1], pts int32 [points_out, 2] in canvas pixels, in drawing order, {lib.FILL_LINK_STATS})"""
        m = None
        if mask is not None:
            m = np.ascontiguousarray(mask, np.uint8)
            if m.ndim != 2:
                raise ValueError(f"mask of shape {m.shape}: [h, w]")
        h, w = (self.H, self.W) if m is None else m.shape
        scal = [int(v) for v in (layer, h, w, *place, reach)]
        if len(scal) != 8:
            raise ValueError("place = (num, den, dx, dy)")
        if any(abs(v) >= 1 << 31 for v in scal):
            raise OripError(f"orip_fill_link: an argument does not fit 32 bits: {scal}")
        st = np.zeros(len(_l.FILL_LINK_STATS), np.int64)
        self._ck(self.L.orip_fill_link(self.h, None if m is None else _p(m), *scal, _p(st)))
        d = {k: int(v) for k, v in zip(_l.FILL_LINK_STATS, st)}
        off = np.zeros(d["paths_out"] + 1, np.int64)
        pts = np.zeros((max(d["points_out"], 1), 2), np.int32)
        self._ck(self.L.orip_fill_link_fetch(self.h, _p(off), _p(pts)))
        return off, pts[:d["points_out"]], d

    def fill_stipple(self, mask, tone, W: int, H: int, place, lattice, clear_rad: int, tone_rad: int, lo: int, hi: int, flags: int, layer: int = 0):
        """fill stipple (include/orip.h: orip_fill_stipple): the dots of a colour mask u8 [h, w] (nonzero = set; None: the resident mask of `layer`, which is
        only read) on the canvas W x H, the mask placed by place = (num, den, dx, dy), on the lattice = (pitch, row, shift) of the whole canvas; a dot keeps
        `clear_rad` source pixels of the mask around it, and the density follows the darkness of tone u8 [h, w] (0 = black; None: all black, the plain
        stipple) over `tone_rad` source pixels, none at darkness `lo` and below, full at `hi` and above; flags: lib.FILL_STIPPLE_SERPENTINE or 0.  Nothing
        resident changes.  -> (xy int32 [dots, 2] in canvas pixels, in drawing order, {lib.FILL_STIPPLE_STATS})"""
        m = None
        if mask is not None:
            m = np.ascontiguousarray(mask, np.uint8)
            if m.ndim != 2:
                raise ValueError(f"mask of shape {m.shape}: [h, w]")
        h, w = (self.H, self.W) if m is None else m.shape
        g = None
        if tone is not None:
            g = np.ascontiguousarray(tone, np.uint8)
            if g.shape != (h, w):
                raise ValueError(f"tone of shape {g.shape} for a mask of {w} x {h}: [h, w]")
        scal = [int(v) for v in (h, w, W, H, *place, *lattice, clear_rad, tone_rad, lo, hi, flags)]
        if len(scal) != 16:
            raise ValueError("place = (num, den, dx, dy) and lattice = (pitch, row, shift)")
        if any(abs(v) >= 1 << 31 for v in scal) or abs(int(layer)) >= 1 << 31:
            raise OripError(f"orip_fill_stipple: an argument does not fit 32 bits: {[int(layer)] + scal}")
        st = np.zeros(len(_l.FILL_STIPPLE_STATS), np.int64)
        self._ck(self.L.orip_fill_stipple(self.h, None if m is None else _p(m), int(layer), None if g is None else _p(g), *scal, _p(st)))
        d = {k: int(v) for k, v in zip(_l.FILL_STIPPLE_STATS, st)}
        xy = np.zeros((max(d["dots"], 1), 2), np.int32)
        self._ck(self.L.orip_fill_stipple_fetch(self.h, _p(xy)))
        return xy[:d["dots"]], d

    def gcode_dash(self, off, pts, pattern, phase, pat_off, pat_val, n: int | None = None):
        """--dashes / --dash-mm (include/orip.h: orip_gcode_dash): of the step polylines (off int64 [n + 1], pts int32 [total, 2]; both None = the n resident
        ones) every stroke with pattern[k] >= 0 is cut into the dashes of that pattern of the table (pat_off int32 [np + 1], pat_val int64, in 1/256 step),
        entered at phase[k]; -1 = solid.  What is left becomes the resident polylines.
        -> (off int64, pts int32 [total', 2], origin int32 [paths_out]: the input stroke of every output stroke, {lib.DASH_STATS})"""
        po, pp, n, _keep = _step_paths(off, pts, n)
        pa = np.ascontiguousarray(pattern, np.int32).reshape(-1)
        ph = np.ascontiguousarray(phase, np.int64).reshape(-1)
        n = len(pa) if n is None else int(n)
        if len(pa) != n or len(ph) != n:
            raise ValueError(f"{len(pa)} patterns and {len(ph)} phases given for {n} paths")
        qo = np.ascontiguousarray(pat_off, np.int32).reshape(-1)
        qv = np.ascontiguousarray(pat_val, np.int64).reshape(-1)
        if len(qo) < 1 or len(qv) < int(qo[-1]):
            raise ValueError(f"{len(qo)} pattern offsets and {len(qv)} entries given")
        st = np.zeros(len(_l.DASH_STATS), np.int64)
        self._ck(self.L.orip_gcode_dash(self.h, po, pp, _p(pa) if n else None, _p(ph) if n else None, n, _p(qo), _p(qv) if len(qv) else None, len(qo) - 1, _p(st)))
        return self._cut_result(st, _l.DASH_STATS, self.L.orip_gcode_dash_fetch)

    def gcode_steps_fetch(self, n: int, total: int, points: bool = True) -> Tuple[np.ndarray, np.ndarray]:
        """the n resident step polylines of `total` points, as gcode_to_steps or gcode_merge left them: (off int64 [n + 1], pts int32 [total, 2]; zeros without `points`)"""
        off = np.zeros(int(n) + 1, np.int64); pts = np.zeros((max(int(total), 1), 2), np.int32)
        self._ck(self.L.orip_gcode_steps_fetch(self.h, _p(off), _p(pts) if points else None))
        return off, pts[:int(total)]

    def gcode_steps_source(self, n: int) -> np.ndarray:
        """for each of the n resident step polylines of gcode_to_steps the index of the input path it came from (int32 [n])"""
        src = np.zeros(max(int(n), 1), np.int32)
        self._ck(self.L.orip_gcode_steps_source_fetch(self.h, _p(src)))
        return src[:int(n)]

    def svg_hatch_groups(self, segments: int) -> np.ndarray:
        """the caller's fill group of every hatch line svg_hatch appended (int32 [segments], the count svg_hatch returned)"""
        out = np.zeros(max(int(segments), 1), np.int32)
        self._ck(self.L.orip_svg_hatch_groups_fetch(self.h, _p(out)))
        return out[:int(segments)]

    def stream_pack(self, table, codes=None) -> bytes:
        """bytes of a piece table (orip.stream.PieceTable) from the resident direction codes; `codes` is what stream_codes(..., fetch_codes=False) returned (None)"""
        if codes is not None:
            raise ValueError("stream_pack reads the codes orip_stream_codes left on the device; pass None")
        c0 = np.ascontiguousarray(table.code0, np.int64); cnt = np.ascontiguousarray(table.cnt, np.int32)
        pos = np.ascontiguousarray(table.pos, np.int64); spd = np.ascontiguousarray(table.speed, np.int32)
        sp = np.ascontiguousarray(table.svc_pos, np.int64); sv = np.ascontiguousarray(table.svc_val, np.uint8)
        npc, ns = len(pos), len(sp)
        self._ck(self.L.orip_stream_pack(self.h, npc, _p(c0) if npc else None, _p(cnt) if npc else None, _p(pos) if npc else None, _p(spd) if npc else None,
                                         ns, _p(sp) if ns else None, _p(sv) if ns else None, int(table.nbytes)))
        out = np.zeros(max(int(table.nbytes), 1), np.uint8)
        self._ck(self.L.orip_stream_pack_fetch(self.h, _p(out)))
        return out[:int(table.nbytes)].tobytes()

    # ---- multi-GPU exchange (RCCL inside liborip.so)
    def comm_unique_id(self) -> bytes:
        buf = (C.c_uint8 * _l.COMM_ID_BYTES)()
        if self.L.orip_comm_unique_id(buf) != 0:
            raise OripError("orip_comm_unique_id failed (RCCL)")
        return bytes(buf)

    def comm_init(self, unique_id: bytes, rank: int, world: int):
        assert len(unique_id) == _l.COMM_ID_BYTES
        buf = (C.c_uint8 * _l.COMM_ID_BYTES).from_buffer_copy(unique_id)
        self._ck(self.L.orip_comm_init(self.h, buf, int(rank), int(world)))

    def comm_destroy(self):
        self._ck(self.L.orip_comm_destroy(self.h))

    def bcast_layer(self, root: int, my_slot: int):
        self._ck(self.L.orip_bcast_layer(self.h, int(root), int(my_slot)))

    def preview_cover(self, slot: int, layer: int, taps_which: int, W: int, H: int, thickness: int, radius: int, antialias: bool):
        """Coverage planes (lines, taps), uint8 (H, W) each, behind the previews 06 / 09 / 11 (include/orip.h: orip_preview_cover; parity unpinned)."""
        lines = np.zeros((H, W), np.uint8); taps = np.zeros((H, W), np.uint8)
        self._ck(self.L.orip_preview_cover(self.h, int(slot), int(layer), int(taps_which), int(W), int(H), int(thickness), int(radius), 1 if antialias else 0, _p(lines), _p(taps)))
        return lines, taps

    def plot_order(self, layer: int, R_insert: float) -> np.ndarray:
        n = C.c_int64(0)
        self._ck(self.L.orip_plot_order(self.h, layer, float(R_insert), C.byref(n)))
        ops = np.zeros((max(n.value, 1), 5), np.int32)
        if n.value:
            self._ck(self.L.orip_get_ops(self.h, layer, _p(ops)))
        return ops[:n.value]
