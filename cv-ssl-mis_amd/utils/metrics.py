"""Binary overlap / surface-distance metrics of the validation path, without medpy.

The reference scores a prediction with ``medpy.metric.binary.dc`` and ``medpy.metric.binary.hd95``
(code/val_2D.py:7-15, code/val_3D.py:82-88).  medpy (pinned by the reference's requirements as ``medpy``, 0.4.0
at the time of the survey) is absent from this image; these functions restate its published algorithm on
numpy/scipy:

  dc   = 2 |A & B| / (|A| + |B|)                                   (0.0 when both are empty)
  hd95 = 95th percentile of the union of the two directed surface-distance sets, a surface voxel being an
         object voxel removed by one binary erosion with the 1-connectivity structuring element, and the
         distance of a surface voxel to the other object's surface coming from the Euclidean distance
         transform of the complement of that surface (``voxelspacing`` = EDT sampling).
"""
import math
import os
import struct

import numpy as np
from scipy.ndimage import binary_erosion, distance_transform_edt, generate_binary_structure


def dc(result, reference):
    result = np.atleast_1d(np.asarray(result).astype(bool))
    reference = np.atleast_1d(np.asarray(reference).astype(bool))
    intersection = np.count_nonzero(result & reference)
    size = np.count_nonzero(result) + np.count_nonzero(reference)
    return 2.0 * intersection / float(size) if size > 0 else 0.0


def _surface_distances(result, reference, voxelspacing=None, connectivity=1):
    result = np.atleast_1d(np.asarray(result).astype(bool))
    reference = np.atleast_1d(np.asarray(reference).astype(bool))
    if not np.any(result):
        raise RuntimeError('The first supplied array does not contain any binary object.')
    if not np.any(reference):
        raise RuntimeError('The second supplied array does not contain any binary object.')
    footprint = generate_binary_structure(result.ndim, connectivity)
    result_border = result ^ binary_erosion(result, structure=footprint, iterations=1)
    reference_border = reference ^ binary_erosion(reference, structure=footprint, iterations=1)
    dt = distance_transform_edt(~reference_border, sampling=voxelspacing)
    return dt[result_border]


def hd95(result, reference, voxelspacing=None, connectivity=1):
    hd1 = _surface_distances(result, reference, voxelspacing, connectivity)
    hd2 = _surface_distances(reference, result, voxelspacing, connectivity)
    return float(np.percentile(np.hstack((hd1, hd2)), 95))


def hd(result, reference, voxelspacing=None, connectivity=1):
    """Hausdorff distance: the larger of the two directed maximum surface distances (medpy.metric.binary.hd) --
    code/test_CNNVIT.py:37 (which names it ``hd95``)."""
    hd1 = _surface_distances(result, reference, voxelspacing, connectivity).max()
    hd2 = _surface_distances(reference, result, voxelspacing, connectivity).max()
    return float(max(hd1, hd2))


def asd(result, reference, voxelspacing=None, connectivity=1):
    """Average surface distance: mean distance of the surface voxels of ``result`` to the surface of ``reference``
    (medpy.metric.binary.asd; not symmetric) -- code/test_3D_util.py:147-152."""
    return float(_surface_distances(result, reference, voxelspacing, connectivity).mean())


def ravd(result, reference):
    """Relative absolute volume difference as medpy defines it: (|result| - |reference|) / |reference| (signed; the
    reference takes abs() of it, code/test_3D_util.py:149)."""
    result = np.atleast_1d(np.asarray(result).astype(bool))
    reference = np.atleast_1d(np.asarray(reference).astype(bool))
    vol_reference = np.count_nonzero(reference)
    if vol_reference == 0:
        raise RuntimeError('The second supplied array does not contain any binary object.')
    return (np.count_nonzero(result) - vol_reference) / float(vol_reference)


# ---- the same scores from the device (mis_hip.ops.surface_metrics) ----------------------------------------------------
# The functions above stay as they are: they are the oracle the device path is tested against (equality, not a tolerance).
_EMPTY_FIRST = 'The first supplied array does not contain any binary object.'
_EMPTY_SECOND = 'The second supplied array does not contain any binary object.'
DEVICE_MAX_EXTENT = 1024          # mis_surface_metrics refuses longer axes (MIS_ERR_UNSUPPORTED)


def device_metrics_enabled():
    """``MIS_DEVICE_METRICS=0`` sends every caller back to the host functions above."""
    return os.environ.get("MIS_DEVICE_METRICS", "1") != "0"


def percentile_from_order_stats(d_lo, d_hi, n, q=95):
    """``np.percentile(x, q)`` (method 'linear') of ``n`` values from the two order statistics it interpolates between:
    ``d_lo = sorted(x)[lo]``, ``d_hi = sorted(x)[min(lo + 1, n - 1)]``, ``lo = floor(q / 100 * (n - 1))``.  numpy's own
    arithmetic, operation for operation (``lib._function_base_impl._lerp``): the virtual index is ONE float64 product, and the
    interpolation switches form at g = 0.5 -- ``a + (b - a) * g`` alone differs from numpy in the last bit on some inputs."""
    virtual = (n - 1) * (q / 100)
    g = virtual - math.floor(virtual)
    diff = d_hi - d_lo
    if g >= 0.5:
        return float(d_hi - diff * (1 - g))
    return float(d_lo + diff * g)


class SurfaceScores:
    """dc / hd95 / hd / asd / asd_rev / ravd of one (prediction, ground truth, class) -- from the device record (decoded on first
    use: one device->host copy of 96 bytes) or, for volumes the kernel refuses, from the host functions.  ``asd`` is
    ``asd(pred, gt)``, ``asd_rev`` is ``asd(gt, pred)``.  Empty masks raise what the host functions raise; ``counts`` and
    ``dc`` never do."""

    def __init__(self, record=None, host=None):
        self._record, self._host, self._fields = record, host, None

    def _f(self):
        if self._fields is None:
            raw = self._record.cpu().numpy().tobytes()
            w = struct.unpack("<7q2d3q", raw)
            self._fields = dict(a=w[0], b=w[1], ab=w[2], sa=w[3], sb=w[4], max_sq=(w[5], w[6]), sum=(w[7], w[8]),
                                sq_lo=w[9], sq_hi=w[10], valid=w[11])
        return self._fields

    @property
    def counts(self):
        """{"a": |A|, "b": |B|, "ab": |A & B|, "sa": |dA|, "sb": |dB|} as Python ints"""
        if self._record is None:
            if self._fields is None:
                self._fields = _host_counts(*self._host)       # two erosions: once
            return self._fields
        f = self._f()
        return {k: f[k] for k in ("a", "b", "ab", "sa", "sb")}

    def _need(self, first, second):
        c = self.counts
        if c[first] == 0:
            raise RuntimeError(_EMPTY_FIRST)
        if c[second] == 0:
            raise RuntimeError(_EMPTY_SECOND)

    @property
    def dc(self):
        c = self.counts
        size = c["a"] + c["b"]
        return 2.0 * c["ab"] / float(size) if size > 0 else 0.0

    @property
    def ravd(self):
        c = self.counts
        if c["b"] == 0:
            raise RuntimeError(_EMPTY_SECOND)
        return (c["a"] - c["b"]) / float(c["b"])

    @property
    def hd95(self):
        if self._record is None:
            return hd95(*self._host)
        self._need("a", "b")
        f = self._f()
        return percentile_from_order_stats(math.sqrt(f["sq_lo"]), math.sqrt(f["sq_hi"]), f["sa"] + f["sb"], 95)

    @property
    def hd(self):
        if self._record is None:
            return hd(*self._host)
        self._need("a", "b")
        return float(max(math.sqrt(self._f()["max_sq"][0]), math.sqrt(self._f()["max_sq"][1])))

    @property
    def asd(self):
        if self._record is None:
            return asd(*self._host)
        self._need("a", "b")
        return self._f()["sum"][0] / self._f()["sa"]

    @property
    def asd_rev(self):
        if self._record is None:
            return asd(self._host[1], self._host[0])
        self._need("b", "a")
        return self._f()["sum"][1] / self._f()["sb"]


def _host_counts(result, reference):
    result, reference = np.asarray(result).astype(bool), np.asarray(reference).astype(bool)

    def border(m):
        return int(np.count_nonzero(m ^ binary_erosion(m, structure=generate_binary_structure(m.ndim, 1)))) if m.any() else 0
    return dict(a=int(np.count_nonzero(result)), b=int(np.count_nonzero(reference)), ab=int(np.count_nonzero(result & reference)),
                sa=border(result), sb=border(reference))


def device_supported(shape):
    """Shapes ``mis_surface_metrics`` takes: 2 or 3 axes, none longer than DEVICE_MAX_EXTENT, no empty axis."""
    return len(shape) in (2, 3) and all(0 < int(e) <= DEVICE_MAX_EXTENT for e in shape)


def device_scores(pred_u8_cuda, gt_u8_cuda, cls):
    """Scores of the masks ``pred == cls`` / ``gt == cls`` (``cls = -1``: label > 0) of two uint8 label maps on the device, as a
    ``SurfaceScores``.  ``dc``, ``hd95``, ``hd`` and ``ravd`` are the host functions' own expressions over the device's integers
    (bit-equal); ``asd`` divides the device's float64 sum (last bits may differ: another summation order).  Nothing is copied
    to the host until a score is read.  Volumes the kernel refuses are scored by the host functions."""
    if not device_supported(tuple(pred_u8_cuda.shape)):
        p, g = pred_u8_cuda.cpu().numpy(), gt_u8_cuda.cpu().numpy()
        return SurfaceScores(host=((p > 0, g > 0) if cls < 0 else (p == cls, g == cls)))
    from mis_hip import ops
    return SurfaceScores(record=ops.surface_metrics(pred_u8_cuda, gt_u8_cuda, cls))


def device_label_map(label):
    """A label map (numpy array or tensor) as a contiguous uint8 device tensor, or None when the device path cannot take it: a
    shape the kernel refuses, or values that are not integers in 0..255 (float arrays with integral values are taken: some
    datasets store their labels so).  The caller scores on the host then."""
    import torch
    arr = label.detach().cpu().numpy() if isinstance(label, torch.Tensor) else np.asarray(label)
    if not device_supported(arr.shape) or not (arr.dtype == np.bool_ or np.issubdtype(arr.dtype, np.integer)
                                               or np.issubdtype(arr.dtype, np.floating)):
        return None
    if arr.dtype != np.bool_ and arr.dtype != np.uint8:
        lo, hi = arr.min(), arr.max()
        if not (lo >= 0 and hi <= 255):                        # also refuses NaN
            return None
        if np.issubdtype(arr.dtype, np.floating) and not np.array_equal(arr, np.rint(arr)):
            return None
    return torch.from_numpy(np.ascontiguousarray(arr).astype(np.uint8)).cuda()
