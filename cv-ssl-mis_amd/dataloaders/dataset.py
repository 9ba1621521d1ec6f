"""2-D (ACDC-style slices) input pipeline on the device.

Mirrors the part of the reference's code/dataloaders/dataset.py that the Mean-Teacher scripts use
(train_mean_teacher_2D.py:167-184): ``BaseDataSets`` (:20-76), ``RandomGenerator`` (:406-425) with
``random_rot_flip`` (:79-89) / ``random_rotate`` (:92-96) and scipy's nearest ``zoom``, ``TwoStreamBatchSampler``
(:247-294).  The training slices are uploaded once into an HBM pool (``DeviceSlicePool``); a batch is then ONE
launch of ``mis_augment2d`` that gathers every output pixel straight from the pool -- what the reference does with
numpy + scipy per sample in DataLoader workers.  The random draws stay on the host and follow the reference's call
order (``random.random()``, ``np.random.randint``), so a seeded run draws the same augmentations; the pixels are
bit-identical to numpy/scipy (tests/test_augment_gpu.py).

On-disk format: the reference reads ``<root>/data/slices/<case>.h5`` with datasets ``image`` / ``label`` through
h5py, which this image does not ship.  ``read_case`` uses h5py when it is importable and otherwise a sibling
``<case>.npz`` with the same two arrays; nothing here re-implements HDF5.
"""
import os
import random

import numpy as np
import torch

from mis_hip import lib as _l

AUG2D_DTYPE = np.dtype([("img_off", "<i8"), ("lab_off", "<i8"), ("H", "<i4"), ("W", "<i4"), ("mode", "<i4"),
                        ("k", "<i4"), ("axis", "<i4"), ("reserved", "<i4"), ("m00", "<f8"), ("m01", "<f8"),
                        ("m10", "<f8"), ("m11", "<f8"), ("off0", "<f8"), ("off1", "<f8")], align=True)
assert AUG2D_DTYPE.itemsize == _l.AUG2D_BYTES


def read_case(path_without_ext):
    """``image`` / ``label`` arrays of one case file (h5 through h5py if available, else .npz)."""
    h5, npz = path_without_ext + ".h5", path_without_ext + ".npz"
    if os.path.exists(h5):
        try:
            import h5py
        except ImportError as e:
            if not os.path.exists(npz):
                raise RuntimeError(f"{h5} needs h5py (not installed); convert it to {npz} with arrays "
                                   "'image' and 'label'") from e
        else:
            with h5py.File(h5, "r") as f:
                return f["image"][:], f["label"][:]
    with np.load(npz) as z:
        return z["image"], z["label"]


class BaseDataSets:
    """Same constructor and item protocol as the reference's BaseDataSets (dataset.py:20-76) for the plain
    (non-CTAugment) path: ``split='train'`` lists ``train_slices.list`` -> ``data/slices/<case>``, ``split='val'``
    lists ``val.list`` -> ``data/<case>``; items are ``{'image', 'label', 'idx'}`` (numpy on the host unless a
    transform turns them into tensors)."""

    def __init__(self, base_dir=None, split="train", num=None, transform=None, ops_weak=None, ops_strong=None):
        assert bool(ops_weak) == bool(ops_strong), \
            "For using CTAugment learned policies, provide both weak and strong batch augmentation policy"
        if ops_weak:
            raise NotImplementedError("CTAugment policies are outside the Mean-Teacher path")
        self._base_dir, self.split, self.transform = base_dir, split, transform
        name = {"train": "train_slices.list", "val": "val.list"}[split]
        with open(os.path.join(base_dir, name)) as f:
            self.sample_list = [ln.replace("\n", "") for ln in f.readlines()]
        if num is not None and split == "train":
            self.sample_list = self.sample_list[:num]
        print("total {} samples".format(len(self.sample_list)))

    def __len__(self):
        return len(self.sample_list)

    def case_path(self, idx):
        sub = "data/slices" if self.split == "train" else "data"
        return os.path.join(self._base_dir, sub, self.sample_list[idx])

    def __getitem__(self, idx):
        image, label = read_case(self.case_path(idx))
        sample = {"image": image, "label": label}
        if self.split == "train" and self.transform is not None:
            sample = self.transform(sample)
        sample["idx"] = idx
        return sample


class DeviceSlicePool:
    """Every training slice resident in HBM: one flat f32 image pool, one flat u8 label pool, per-slice
    (offset, H, W).  ACDC's 1 902 slices are ~0.6 GB; the pool is sized by the data, not by a cache policy."""

    def __init__(self, slices):
        """``slices``: iterable of (image [H,W] float, label [H,W] integer) numpy arrays."""
        imgs, labs, self.shapes, self.offsets = [], [], [], []
        off = 0
        for image, label in slices:
            image = np.asarray(image)
            assert image.ndim == 2 and tuple(label.shape) == tuple(image.shape)
            imgs.append(np.ascontiguousarray(image, dtype=np.float32).ravel())
            labs.append(np.ascontiguousarray(label).astype(np.uint8).ravel())
            self.shapes.append(tuple(image.shape))
            self.offsets.append(off)
            off += image.size
        if not imgs:
            raise ValueError("empty slice pool")
        self.img = torch.from_numpy(np.concatenate(imgs)).cuda()
        self.lab = torch.from_numpy(np.concatenate(labs)).cuda()

    @classmethod
    def from_dataset(cls, ds):
        return cls(read_case(ds.case_path(i)) for i in range(len(ds)))

    def __len__(self):
        return len(self.shapes)


def rotate_params(angle, shape):
    """scipy.ndimage.rotate's affine parameters for a 2-D array (scipy/ndimage/_interpolation.py, reshape=False):
    rot_matrix = [[cosdg, sindg], [-sindg, cosdg]], offset = in_center - rot_matrix @ out_center."""
    from scipy import special
    c, s = special.cosdg(angle), special.sindg(angle)
    m = np.array([[c, s], [-s, c]])
    plane = np.asarray(shape, dtype=np.int64)
    out_center = m @ ((plane - 1) / 2)
    in_center = (plane - 1) / 2
    off = in_center - out_center
    return m, off


class RandomGenerator:
    """The reference's RandomGenerator (dataset.py:406-425) split into its random draws (host, same call order)
    and its pixel work (device).  ``draw`` returns (mode, k, axis, angle)."""

    def __init__(self, output_size):
        self.output_size = tuple(int(v) for v in output_size)

    def draw(self):
        if random.random() > 0.5:                      # :413-414 random_rot_flip
            k = np.random.randint(0, 4)
            axis = np.random.randint(0, 2)
            return 1, int(k), int(axis), 0
        elif random.random() > 0.5:                    # :415-416 random_rotate
            return 2, 0, 0, int(np.random.randint(-20, 20))
        return 0, 0, 0, 0

    def fill(self, rec, pool, idx):
        """Draw for slice ``idx`` of ``pool`` and write its MisAug2D record."""
        mode, k, axis, angle = self.draw()
        H, W = pool.shapes[idx]
        rec["img_off"] = rec["lab_off"] = pool.offsets[idx]
        rec["H"], rec["W"], rec["mode"], rec["k"], rec["axis"] = H, W, mode, k, axis
        if mode == 2:
            m, off = rotate_params(angle, (H, W))
            rec["m00"], rec["m01"], rec["m10"], rec["m11"] = m[0, 0], m[0, 1], m[1, 0], m[1, 1]
            rec["off0"], rec["off1"] = off[0], off[1]
        return mode, k, axis, angle

    def __call__(self, sample):
        """Drop-in item transform: one slice through the same device kernel; returns device tensors
        ``image`` f32 [1,h,w] and ``label`` u8 [h,w] (the reference returns the CPU equivalents)."""
        pool = DeviceSlicePool([(sample["image"], sample["label"])])
        image, label = augment_batch(pool, [0], self)
        return {"image": image[0], "label": label[0]}


def augment_batch(pool, indices, gen, recs=None, out=None):
    """One launch: slices ``indices`` of ``pool`` -> (image [B,1,h,w] f32, label [B,h,w] u8) on the device.
    ``recs``: pinned uint8 staging tensor of >= B records (allocated if None); ``out``: reusable output pair."""
    if hasattr(gen, "augment"):            # a transform of more than one launch (WeakStrongAugment)
        return gen.augment(pool, indices, recs=recs, out=out)
    B = len(indices)
    h, w = gen.output_size
    if recs is None:
        recs = torch.empty(B * _l.AUG2D_BYTES, dtype=torch.uint8).pin_memory()
    host = recs.numpy()[:B * _l.AUG2D_BYTES].view(AUG2D_DTYPE)
    host[:] = 0
    for b, idx in enumerate(indices):
        gen.fill(host[b], pool, int(idx))
    dev = recs[:B * _l.AUG2D_BYTES].cuda(non_blocking=True)
    if out is None:
        out = (torch.empty((B, 1, h, w), dtype=torch.float32, device="cuda"),
               torch.empty((B, h, w), dtype=torch.uint8, device="cuda"))
    _l.launch("mis_augment2d", pool.img, pool.lab, dev, B, h, w, out[0], out[1])
    return out


class _Resize:
    """``zoom(.., order=0)`` to ``output_size`` alone (MisAug2D mode 0)."""

    def __init__(self, output_size):
        self.output_size = output_size

    def fill(self, rec, pool, idx):
        H, W = pool.shapes[idx]
        rec["img_off"] = rec["lab_off"] = pool.offsets[idx]
        rec["H"], rec["W"] = H, W


class RandomGenerator_w(_Resize):
    """The reference's RandomGenerator_w (dataset.py:196-208), the weak transform of the contrastive cross-teaching
    scripts: ``zoom(.., order=0)`` of image and label to ``output_size`` and nothing else -- no draw, no rotation, no flip."""

    def __init__(self, output_size):
        super().__init__(tuple(int(v) for v in output_size))

    def __call__(self, sample):
        """Drop-in item transform (device tensors ``image`` f32 [1,h,w] and ``label`` u8 [h,w])."""
        pool = DeviceSlicePool([(sample["image"], sample["label"])])
        image, label = augment_batch(pool, [0], self)
        return {"image": image[0], "label": label[0]}


class _RotFlip(_Resize):
    """``random_rot_flip`` (MisAug2D mode 1) with the reference's draws, on slices that already have the output size."""

    def fill(self, rec, pool, idx):
        super().fill(rec, pool, idx)
        k = np.random.randint(0, 4)                    # dataset.py:80
        axis = np.random.randint(0, 2)                 # dataset.py:82
        rec["mode"], rec["k"], rec["axis"] = 1, int(k), int(axis)


class _ResizedPool:
    """A batch of equally sized device slices (image [B,1,h,w] f32, label [B,h,w] u8) seen as a slice pool."""

    def __init__(self, image, label):
        B, _, h, w = image.shape
        self.img, self.lab = image.reshape(-1), label.reshape(-1)
        self.shapes, self.offsets = [(h, w)] * B, [b * h * w for b in range(B)]


class WeakStrongAugment:
    """The reference's WeakStrongAugment (dataset.py:211-245) on the device.  Per slice, in the reference's order: resize
    (``zoom(order=0)``), then the weak augmentation ``random_rot_flip`` -- always, never the +-20 degree rotation -- with host
    draws in the reference's call order (``k = np.random.randint(0, 4)``, ``axis = np.random.randint(0, 2)``): two launches
    of ``mis_augment2d`` per batch (resize, then rotate / flip the resized slices; a non-square patch is resized once more
    after an odd rotation, where the reference would return a transposed image).  The strong augmentation is colour jitter
    (``mis_color_jitter``): as a batch transform of the training loader this class yields the weak batch and the labels, and
    ``FixMatchTrainer`` draws the jitter factors on the device; as an item transform it draws them on the host in
    torchvision's order (``ColorJitter.get_params``: a permutation of the four adjustments from torch's generator, then one
    uniform factor each) and returns ``image``, ``image_weak``, ``image_strong`` (f32 [1,h,w]) and ``label_aug`` (u8 [h,w])
    device tensors."""

    def __init__(self, output_size):
        self.output_size = tuple(int(v) for v in output_size)

    def augment(self, pool, indices, recs=None, out=None, keep_resized=False):
        B = len(indices)
        resized = augment_batch(pool, indices, _Resize(self.output_size), recs=recs)
        # pageable staging of its own: the first launch's records may still be in flight in ``recs``
        staged = torch.zeros(B * _l.AUG2D_BYTES, dtype=torch.uint8)
        weak = augment_batch(_ResizedPool(*resized), list(range(B)), _RotFlip(self.output_size), recs=staged, out=out)
        return (weak, resized) if keep_resized else weak

    @staticmethod
    def draw_jitter():
        """(beta, gamma, order) with the generator consumption of torchvision's ColorJitter.get_params."""
        fn_idx = torch.randperm(4).tolist()
        beta = float(torch.empty(1).uniform_(0.2, 1.8))        # brightness 0.8
        gamma = float(torch.empty(1).uniform_(0.2, 1.8))       # contrast 0.8
        torch.empty(1).uniform_(0.2, 1.8)                      # saturation 0.8: no effect on one channel
        torch.empty(1).uniform_(-0.2, 0.2)                     # hue 0.2: no effect on one channel
        return beta, gamma, int(fn_idx.index(1) < fn_idx.index(0))

    def __call__(self, sample):
        from mis_hip import ops
        pool = DeviceSlicePool([(sample["image"], sample["label"])])
        (weak, label), (image, _) = self.augment(pool, [0], keep_resized=True)
        params = torch.tensor([self.draw_jitter()], dtype=torch.float32, device="cuda")
        strong = torch.empty_like(weak)
        ops.color_jitter(weak, strong, params=params)
        return {"image": image[0], "image_weak": weak[0], "image_strong": strong[0], "label_aug": label[0]}


class TwoStreamBatchSampler:
    """Index batches ``labeled + unlabeled`` -- labeled samples FIRST (the contract the step relies on, SURVEY s.8
    row a13).  Same constructor, length and random-number consumption as the reference's sampler
    (dataset.py:247-294): an epoch is one ``np.random.permutation`` pass over the primary (labeled) indices in
    chunks of ``batch_size - secondary_batch_size`` (a ragged tail is dropped); the secondary (unlabeled) indices are
    consumed from an endless sequence of fresh permutations, a new one being drawn only when the previous is used up."""

    def __init__(self, primary_indices, secondary_indices, batch_size, secondary_batch_size):
        self.primary_indices = primary_indices
        self.secondary_indices = secondary_indices
        self.secondary_batch_size = secondary_batch_size
        self.primary_batch_size = batch_size - secondary_batch_size
        assert len(self.primary_indices) >= self.primary_batch_size > 0
        assert len(self.secondary_indices) >= self.secondary_batch_size > 0

    def __iter__(self):
        labeled = np.random.permutation(self.primary_indices)       # drawn when the epoch starts
        nl, nu = self.primary_batch_size, self.secondary_batch_size
        stock = []                                                  # unread part of the current unlabeled shuffle
        for start in range(0, len(labeled) - nl + 1, nl):
            unlabeled = []
            while len(unlabeled) < nu:
                if not stock:
                    stock = list(np.random.permutation(self.secondary_indices))
                need = nu - len(unlabeled)
                unlabeled += stock[:need]
                stock = stock[need:]
            yield tuple(labeled[start:start + nl]) + tuple(unlabeled)

    def __len__(self):
        return len(self.primary_indices) // self.primary_batch_size


class DeviceTwoStreamLoader:
    """``DataLoader(db_train, batch_sampler=TwoStreamBatchSampler(...))`` with the dataset in HBM: iterating yields
    ``{'image': f32 [B,1,h,w], 'label': u8 [B,h,w]}`` device tensors, one gather launch per batch.  A small ring of
    pinned parameter buffers lets the host run ahead of the device without overwriting records in flight."""

    RING = 4

    def __init__(self, pool, batch_sampler, transform):
        self.pool, self.batch_sampler, self.transform = pool, batch_sampler, transform
        B = batch_sampler.primary_batch_size + batch_sampler.secondary_batch_size
        self._recs = [torch.empty(B * _l.AUG2D_BYTES, dtype=torch.uint8).pin_memory() for _ in range(self.RING)]
        self._events = [None] * self.RING
        self._i = 0

    def __len__(self):
        return len(self.batch_sampler)

    def __iter__(self):
        for batch in self.batch_sampler:
            slot = self._i % self.RING
            self._i += 1
            if self._events[slot] is not None:
                self._events[slot].synchronize()
            image, label = augment_batch(self.pool, batch, self.transform, recs=self._recs[slot])
            ev = torch.cuda.Event()
            ev.record()
            self._events[slot] = ev
            yield {"image": image, "label": label}


def zoom_slices(stack, out_size):
    """Nearest-neighbour resize of every slice of a device tensor ``stack`` [Z, H, W] (f32) to ``out_size`` --
    ``scipy.ndimage.zoom(slice, (oh / H, ow / W), order=0)`` for all Z slices in one ``mis_augment2d`` launch
    (mode 0: no augmentation).  Returns [Z, 1, oh, ow] f32 on the device."""
    assert stack.dim() == 3 and stack.dtype == torch.float32 and stack.is_cuda and stack.is_contiguous()
    Z, H, W = stack.shape
    oh, ow = (int(v) for v in out_size)
    host = np.zeros(Z, AUG2D_DTYPE)
    host["img_off"] = np.arange(Z, dtype=np.int64) * (H * W)
    host["H"], host["W"] = H, W
    dev = torch.from_numpy(host.view(np.uint8)).cuda()
    out = torch.empty((Z, 1, oh, ow), dtype=torch.float32, device="cuda")
    _l.launch("mis_augment2d", stack, None, dev, Z, oh, ow, out, None)
    return out
