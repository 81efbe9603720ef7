"""A track table that lives in device memory.

``rx.track.TrackSet`` is a host object: even its "device" backend downloads the
table rx_build_tracks wrote, walks it on the host and hands host arrays to
rx_upload_tracks, which derives the culling tables in a host loop and uploads
everything again.  ``DeviceTrackTable`` keeps the four arrays where the kernel
left them; ``RacingVectorEnv.set_tracks`` hands them to rx_upload_tracks_device,
which copies them device to device and builds the culling tables with a kernel
(include/rx.h, csrc/rx_cull.hip).  Only the [n + 1] offsets and the control
points exist on the host; the table itself comes down when someone asks for it
(``download``, ``track_set``: the renderer, ``save_table``).

The table is the C level's, unchanged: meta[:, 2] and meta[:, 4] are
rx_build_tracks' values (ocml atan2, x * x), which ``TrackSet`` replaces by the
reference's numpy expressions.  ``from_arrays`` uploads a
``TrackSet.arrays()`` dict as it is, so an env swapped onto it steps bit for bit
like one constructed on that TrackSet.
"""
import ctypes

import numpy as np
import torch

from . import _lib
from .track import DEFAULT_CONTROL_POINTS, DEFAULT_WIDTH, TrackSet

KEYS = ("wp", "nrm", "seg", "meta")


class DeviceTrackTable:
    """Slots packed as rx_upload_tracks' layout, the arrays on ``device``:
    ``wp_off`` (host int32 [n + 1]), ``wp`` / ``nrm`` [Wtot, 2], ``seg``
    [2 Wtot, 4], ``meta`` [n, 8] (float64 tensors), plus what the host knows of
    the slots: ``control_points``, ``widths`` (None when built ``from_arrays``
    without them) and ``factor``."""

    def __init__(self, wp_off, wp, nrm, seg, meta, control_points=None, widths=None, factor=30):
        self.wp_off = np.ascontiguousarray(wp_off, dtype=np.int32)
        self.wp, self.nrm, self.seg, self.meta = wp, nrm, seg, meta
        self.device = meta.device
        self._control_points, self._widths, self.factor = control_points, widths, factor
        self._cp_dev = None  # build_from_device: (cp_off, cp, width), downloaded when someone asks
        self._track_set = None

    def _download_control_points(self):
        cp_off, cp_d, w_d = self._cp_dev
        cp = cp_d.cpu().numpy().reshape(-1, 2)
        self._control_points = [cp[cp_off[k]:cp_off[k + 1]].copy() for k in range(len(cp_off) - 1)]
        self._widths = [float(w) for w in w_d.cpu().numpy()]
        self._cp_dev = None

    @property
    def control_points(self):
        if self._cp_dev is not None:
            self._download_control_points()
        return self._control_points

    @control_points.setter
    def control_points(self, value):
        self._control_points = value

    @property
    def widths(self):
        if self._cp_dev is not None:
            self._download_control_points()
        return self._widths

    @widths.setter
    def widths(self, value):
        self._widths = value

    def __len__(self):
        return len(self.wp_off) - 1

    @classmethod
    def build(cls, control_points, widths, factor=30, device=None):
        """One slot per given track, in order, no dedup: ONE rx_build_tracks launch
        on torch's current stream of ``device``, no download and no wait.  What the
        host can see is checked here (RxError names the track and the field); a
        track only device memory shows to be bad (a repeated control point, a
        non-finite coordinate, a negative width) is marked by the kernel and refused
        by ``RacingVectorEnv.set_tracks``."""
        L = _lib.load()
        dev = torch.device("cuda" if device is None else device)
        if dev.index is None:
            dev = torch.device("cuda", torch.cuda.current_device())
        cps = [DEFAULT_CONTROL_POINTS if c is None else c for c in control_points]
        ws = [DEFAULT_WIDTH if w is None else w for w in widths]
        n = len(cps)
        if n == 0 or len(ws) != n:
            raise ValueError("need at least one track and one width per track")
        flat = [np.asarray(c, dtype=np.float64) for c in cps]
        for k, c in enumerate(flat):
            if c.ndim != 2 or c.shape[1] != 2:
                raise ValueError(f"track {k}: control points must be [P, 2], got {c.shape}")
        cp_off = np.concatenate([[0], np.cumsum([len(c) for c in flat])]).astype(np.int32)
        cp = np.ascontiguousarray(np.concatenate(flat))
        w = np.ascontiguousarray(ws, dtype=np.float64)
        wt = max(int(cp_off[-1]) * max(int(factor), 0), 0)
        cuts = np.concatenate([[0], np.cumsum((2 * wt, 2 * wt, 8 * wt, 8 * n))])
        wp_off = np.zeros(n + 1, dtype=np.int32)
        with torch.cuda.device(dev):
            cp_d, w_d = torch.from_numpy(cp).to(dev), torch.from_numpy(w).to(dev)
            flat_d = torch.empty(int(cuts[-1]), dtype=torch.float64, device=dev)
            parts = [flat_d[cuts[i]:cuts[i + 1]] for i in range(4)]
            _lib.check(L.rx_build_tracks(n, factor, _lib.ptr(cp_off), _lib.ptr(cp_d), _lib.ptr(w_d), _lib.ptr(wp_off),
                                         *[_lib.ptr(x) for x in parts], _lib.stream_ptr()), "rx_build_tracks")
        return cls(wp_off, parts[0].view(wt, 2), parts[1].view(wt, 2), parts[2].view(2 * wt, 4), parts[3].view(n, 8),
                   control_points=cps, widths=ws, factor=factor)

    @classmethod
    def build_from_device(cls, cp_off, cp_d, width_d, factor=30):
        """``build`` on control points that already live in device memory: ``cp_off``
        (host int32 [n + 1], in points), ``cp_d`` (float64 [cp_off[n], 2]) and
        ``width_d`` (float64 [n]) on one device.  The same ONE rx_build_tracks launch
        on torch's current stream, without the host concatenation and the upload; no
        download and no wait.  ``control_points`` and ``widths`` come down only when
        ``track_set()`` or a caller asks for them (the tensors are kept until then)."""
        L = _lib.load()
        cp_off = np.ascontiguousarray(cp_off, dtype=np.int32)
        n, dev = len(cp_off) - 1, width_d.device
        if n <= 0:
            raise ValueError("need at least one track and one width per track")
        if cp_d.device != dev or dev.type != "cuda" or cp_d.dtype != torch.float64 or width_d.dtype != torch.float64 \
                or tuple(cp_d.shape) != (int(cp_off[-1]), 2) or tuple(width_d.shape) != (n,) \
                or not cp_d.is_contiguous() or not width_d.is_contiguous():
            raise ValueError(f"build_from_device: need contiguous float64 control points [{int(cp_off[-1])}, 2] and "
                             f"widths [{n}] on one cuda device, got {tuple(cp_d.shape)} {cp_d.dtype} on {cp_d.device} "
                             f"and {tuple(width_d.shape)} {width_d.dtype} on {dev}")
        wt = max(int(cp_off[-1]) * max(int(factor), 0), 0)
        cuts = np.concatenate([[0], np.cumsum((2 * wt, 2 * wt, 8 * wt, 8 * n))])
        wp_off = np.zeros(n + 1, dtype=np.int32)
        with torch.cuda.device(dev):
            flat_d = torch.empty(int(cuts[-1]), dtype=torch.float64, device=dev)
            parts = [flat_d[cuts[i]:cuts[i + 1]] for i in range(4)]
            _lib.check(L.rx_build_tracks(n, factor, _lib.ptr(cp_off), _lib.ptr(cp_d), _lib.ptr(width_d),
                                         _lib.ptr(wp_off), *[_lib.ptr(x) for x in parts], _lib.stream_ptr()),
                       "rx_build_tracks")
        table = cls(wp_off, parts[0].view(wt, 2), parts[1].view(wt, 2), parts[2].view(2 * wt, 4), parts[3].view(n, 8),
                    factor=factor)
        table._cp_dev = (cp_off, cp_d, width_d)
        return table

    @classmethod
    def from_arrays(cls, arrays, device):
        """Upload a packed host table (``TrackSet.arrays()``: wp_off, wp, nrm, seg,
        meta) unchanged.  The control points are not part of it: ``track_set()``
        then gives slots without them (widths from meta[:, 3])."""
        dev = torch.device(device)
        up = {k: torch.from_numpy(np.ascontiguousarray(arrays[k], dtype=np.float64)).to(dev) for k in KEYS}
        return cls(arrays["wp_off"], up["wp"], up["nrm"], up["seg"], up["meta"])

    @staticmethod
    def patch(source):
        """The rx_track_patch struct that puts ``source`` (``replacement``'s table)
        into its ``slots``, and the arrays it points to: keep the second value
        alive until the call that takes the struct returns."""
        keep = (source.slots, source.wp_off, source.wp, source.nrm, source.seg, source.meta)
        return _lib.RxTrackPatch(len(source.slots), *[_lib.ptr(x) for x in keep]), keep

    def replacement(self, slots, control_points, widths):
        """The first half of ``replace``: the checks, then the small table of the new
        tracks (``build``: one rx_build_tracks launch), in ascending slot order; its
        ``slots`` attribute holds those slots (int32), row for row.  Nothing of this
        table changes."""
        slots = np.asarray(slots, dtype=np.int64).reshape(-1)
        n = len(self)
        if len(slots) == 0 or len(control_points) != len(slots) or len(widths) != len(slots):
            raise ValueError("replace: need at least one slot, and one track and one width per slot")
        if slots.min() < 0 or slots.max() >= n or len(np.unique(slots)) != len(slots):
            raise ValueError(f"replace: the slots must be distinct and lie in [0, {n})")
        order = np.argsort(slots, kind="stable")
        slots = slots[order]
        cps = [DEFAULT_CONTROL_POINTS if control_points[i] is None else control_points[i] for i in order]
        ws = [DEFAULT_WIDTH if widths[i] is None else widths[i] for i in order]
        for k, c in zip(slots, cps):
            have, want = len(c) * self.factor, int(self.wp_off[k + 1] - self.wp_off[k])
            if have != want:
                raise ValueError(f"replace: slot {k} has {want} waypoints ({want / self.factor:g} control points x "
                                 f"{self.factor}), its new track {len(c)} control points: a replaced slot keeps its "
                                 "point count")
        source = DeviceTrackTable.build(cps, ws, factor=self.factor, device=self.device)
        source.slots = np.ascontiguousarray(slots, dtype=np.int32)
        return source

    def replacement_from_device(self, slots, out_off, cp_d, width_d):
        """``replacement`` for new tracks that already live in device memory: row j of
        ``out_off`` (host int32 [n + 1], in points), ``cp_d`` (float64 [out_off[n], 2]) and
        ``width_d`` (float64 [n]) goes into ``slots[j]``; the slots must be ascending.  The same
        checks from the host offsets (ValueError naming the slot whose span is not its point
        count), then ``build_from_device``: one rx_build_tracks launch, no upload, no download."""
        slots = np.asarray(slots, dtype=np.int64).reshape(-1)
        out_off = np.ascontiguousarray(out_off, dtype=np.int32).reshape(-1)
        n = len(self)
        if len(slots) == 0 or len(out_off) != len(slots) + 1:
            raise ValueError("replace: need at least one slot, and one row of offsets per slot and one more")
        if slots.min() < 0 or slots.max() >= n or np.any(np.diff(slots) <= 0):
            raise ValueError(f"replace: the slots must be distinct, ascending and lie in [0, {n})")
        for k, have in zip(slots, np.diff(out_off)):
            want = int(self.wp_off[k + 1] - self.wp_off[k])
            if int(have) * self.factor != want:
                raise ValueError(f"replace: slot {k} has {want} waypoints ({want / self.factor:g} control points x "
                                 f"{self.factor}), its new track {int(have)} control points: a replaced slot keeps its "
                                 "point count")
        source = DeviceTrackTable.build_from_device(out_off, cp_d, width_d, factor=self.factor)
        source.slots = np.ascontiguousarray(slots, dtype=np.int32)
        return source

    def apply(self, source):
        """The second half of ``replace``: ``source``'s rows written over its slots'
        rows of this table (rx_patch_tracks: one launch on torch's current stream, no
        wait, no download), and the control points and widths this table knows.  A
        source whose control points live in device memory (``replacement_from_device``)
        is not downloaded for that: this table then knows no control points until
        ``point_at`` names the buffer that holds the pool."""
        p, keep = self.patch(source)
        with torch.cuda.device(self.device):
            _lib.check(_lib.load().rx_patch_tracks(len(self), _lib.ptr(self.wp_off), _lib.ptr(self.wp),
                                                   _lib.ptr(self.nrm), _lib.ptr(self.seg), _lib.ptr(self.meta), 0, 0,
                                                   None, ctypes.byref(p), _lib.stream_ptr()), "rx_patch_tracks")
        del keep
        if source._cp_dev is not None:
            self._control_points = self._widths = self._cp_dev = None
        elif self.control_points is not None:  # (a build_from_device table downloads them here)
            for k, c, w in zip(source.slots, source.control_points, source.widths):
                self._control_points[k], self._widths[k] = c, w
        self._track_set = None

    def point_at(self, cp_off, cp_d, width_d):
        """The control points of this table's slots are the device buffer (``cp_off`` host
        int32 [n + 1], ``cp_d`` float64 [cp_off[n], 2], ``width_d`` float64 [n]) from now on:
        ``control_points`` / ``widths`` download it when asked, as after ``build_from_device``."""
        if len(cp_off) != len(self) + 1:
            raise ValueError(f"point_at: {len(cp_off) - 1} slots of control points for a table of {len(self)}")
        self._control_points = self._widths = self._track_set = None
        self._cp_dev = (np.ascontiguousarray(cp_off, dtype=np.int32), cp_d, width_d)

    def replace(self, slots, control_points, widths):
        """New tracks in the given slots of this table, in place.  A slot keeps its
        waypoint count, so every offset and address stays: a track whose point count
        differs from its slot's is refused (ValueError naming the slot) before
        anything is built.  ``slots`` must be distinct; they are taken in ascending
        order with their tracks.  Returns the small source table (``replacement``).
        A track only device memory shows to be bad is copied as it is, NaN mark
        included: ``RacingVectorEnv.replace_tracks`` refuses it before it gets here."""
        source = self.replacement(slots, control_points, widths)
        self.apply(source)
        return source

    def download(self):
        """The raw table as a dict of host arrays (rx_upload_tracks' layout)."""
        out = {k: getattr(self, k).cpu().numpy() for k in KEYS}
        return dict(wp_off=self.wp_off.copy(), **out)

    def track_set(self):
        """A ``TrackSet`` of backend "device" over the downloaded table (through
        ``TrackSet._adopt``, so a slot equals ``TrackGeometry.from_waypoints`` of its
        waypoints); the download happens on first use only."""
        if self._track_set is None:
            a = self.download()
            n = len(self)
            cps = self.control_points if self.control_points is not None else [None] * n
            ws = self.widths if self.widths is not None else [float(x) for x in a["meta"][:, 3]]
            ts = TrackSet(self.factor, "device")
            ts.device = self.device
            ts._adopt(list(zip(cps, ws)), a)
            for k, (c, w) in enumerate(zip(cps, ws)):
                if c is not None:
                    ts._index.setdefault(TrackSet._key(c, w), k)
            self._track_set = ts
        return self._track_set
