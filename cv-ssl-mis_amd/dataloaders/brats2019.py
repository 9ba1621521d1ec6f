"""3-D (BraTS-style volumes) input pipeline on the device.

Mirrors what train_mean_teacher_3D.py:98-114 uses from the reference's code/dataloaders/brats2019.py:
``BraTS2019`` (:13-46), ``Compose([RandomRotFlip(), RandomCrop(patch_size), ToTensor()])`` (:84-147,196-208) and the
two-stream sampler (same class as the 2-D one).  The volumes are uploaded once into an HBM pool -- 250 BraTS volumes
of 240x240x155 are ~11 GB as f32 + u8, a small part of 288 GB -- and a batch is ONE ``mis_crop_rotflip3d`` launch:
every output voxel is gathered from rot90/flip/zero-pad/crop index arithmetic, so the host never touches a voxel.
The random draws (``np.random.randint``) stay on the host in the reference's order.
"""
import os

import numpy as np
import torch

from mis_hip import lib as _l

from .dataset import TwoStreamBatchSampler, read_case   # noqa: F401  (re-exported like the reference module)

CROP3D_DTYPE = np.dtype([("img_off", "<i8"), ("lab_off", "<i8"), ("d0", "<i4"), ("d1", "<i4"), ("d2", "<i4"),
                         ("k", "<i4"), ("axis", "<i4"), ("o0", "<i4"), ("o1", "<i4"), ("o2", "<i4")], align=True)
assert CROP3D_DTYPE.itemsize == _l.CROP3D_BYTES


class BraTS2019:
    """Same constructor / item protocol as the reference's BraTS2019 (brats2019.py:13-46): ``train.txt`` / ``val.txt``
    list the cases, each ``data/<case>`` holds ``image`` and ``label`` (label cast to uint8)."""

    def __init__(self, base_dir=None, split='train', num=None, transform=None):
        self._base_dir, self.transform = base_dir, transform
        with open(os.path.join(base_dir, {'train': 'train.txt', 'test': 'val.txt'}[split])) as f:
            self.image_list = [ln.replace('\n', '').split(",")[0] for ln in f.readlines()]
        if num is not None:
            self.image_list = self.image_list[:num]
        print("total {} samples".format(len(self.image_list)))

    def __len__(self):
        return len(self.image_list)

    def case_path(self, idx):
        return os.path.join(self._base_dir, "data", self.image_list[idx])

    def __getitem__(self, idx):
        image, label = read_case(self.case_path(idx))
        sample = {'image': image, 'label': label.astype(np.uint8)}
        if self.transform:
            sample = self.transform(sample)
        return sample


class DeviceVolumePool:
    """Every training volume resident in HBM (flat f32 image pool + flat u8 label pool, per-volume offset/shape)."""

    def __init__(self, volumes):
        imgs, labs, self.shapes, self.offsets = [], [], [], []
        off = 0
        for image, label in volumes:
            image = np.asarray(image)
            assert image.ndim == 3 and tuple(label.shape) == tuple(image.shape)
            imgs.append(torch.from_numpy(np.ascontiguousarray(image, dtype=np.float32).ravel()))
            labs.append(torch.from_numpy(np.ascontiguousarray(label).astype(np.uint8).ravel()))
            self.shapes.append(tuple(image.shape))
            self.offsets.append(off)
            off += image.size
        if not imgs:
            raise ValueError("empty volume pool")
        self.img = torch.cat(imgs).cuda()
        self.lab = torch.cat(labs).cuda()

    @classmethod
    def from_dataset(cls, ds):
        return cls(read_case(ds.case_path(i)) for i in range(len(ds)))

    def __len__(self):
        return len(self.shapes)


class RandomRotFlipCrop:
    """``RandomRotFlip()`` followed by ``RandomCrop(output_size)`` (brats2019.py:134-147, :84-131) as random draws:
    k = randint(0, 4), axis = randint(0, 2); then, on the rotated shape, the reference zero-pads every axis by
    ``max((out - dim) // 2 + 3, 0)`` on both sides if ANY axis is <= its output size (:99-108) and draws the crop
    origin ``randint(0, padded_dim - out)`` per axis (:115-117)."""

    def __init__(self, output_size):
        self.output_size = tuple(int(v) for v in output_size)

    def draw(self, shape):
        k = int(np.random.randint(0, 4))
        axis = int(np.random.randint(0, 2))
        w, h, d = (shape[1], shape[0], shape[2]) if k & 1 else shape
        out = self.output_size
        pads = (0, 0, 0)
        if w <= out[0] or h <= out[1] or d <= out[2]:
            pads = tuple(max((out[i] - dim) // 2 + 3, 0) for i, dim in enumerate((w, h, d)))
        w, h, d = w + 2 * pads[0], h + 2 * pads[1], d + 2 * pads[2]
        w1 = int(np.random.randint(0, w - out[0]))
        h1 = int(np.random.randint(0, h - out[1]))
        d1 = int(np.random.randint(0, d - out[2]))
        return k, axis, (w1 - pads[0], h1 - pads[1], d1 - pads[2])

    def fill(self, rec, pool, idx):
        shape = pool.shapes[idx]
        k, axis, origin = self.draw(shape)
        rec["img_off"] = rec["lab_off"] = pool.offsets[idx]
        rec["d0"], rec["d1"], rec["d2"] = shape
        rec["k"], rec["axis"] = k, axis
        rec["o0"], rec["o1"], rec["o2"] = origin
        return k, axis, origin


def crop_batch(pool, indices, gen, recs=None, out=None, label_dtype=torch.int64):
    """One launch: volumes ``indices`` -> (image [B,1,p0,p1,p2] f32, label [B,p0,p1,p2] int64 | uint8) on the device
    (ToTensor's layout, brats2019.py:196-208)."""
    B = len(indices)
    p = gen.output_size
    if recs is None:
        recs = torch.empty(B * _l.CROP3D_BYTES, dtype=torch.uint8).pin_memory()
    host = recs.numpy()[:B * _l.CROP3D_BYTES].view(CROP3D_DTYPE)
    host[:] = 0
    for b, idx in enumerate(indices):
        gen.fill(host[b], pool, int(idx))
    dev = recs[:B * _l.CROP3D_BYTES].cuda(non_blocking=True)
    if out is None:
        out = (torch.empty((B, 1) + p, dtype=torch.float32, device="cuda"),
               torch.empty((B,) + p, dtype=label_dtype, device="cuda"))
    assert out[1].dtype in (torch.int64, torch.uint8)
    _l.launch("mis_crop_rotflip3d", pool.img, pool.lab, dev, B, p[0], p[1], p[2], out[0], out[1],
              8 if out[1].dtype == torch.int64 else 1)
    return out


class DeviceTwoStreamLoader3D:
    """``DataLoader(BraTS2019(..., transform=Compose([RandomRotFlip(), RandomCrop(p), ToTensor()])),
    batch_sampler=TwoStreamBatchSampler(...))`` with the dataset in HBM; yields device tensors."""

    RING = 4

    def __init__(self, pool, batch_sampler, transform, label_dtype=torch.int64):
        self.pool, self.batch_sampler, self.transform, self.label_dtype = pool, batch_sampler, transform, label_dtype
        B = batch_sampler.primary_batch_size + batch_sampler.secondary_batch_size
        self._recs = [torch.empty(B * _l.CROP3D_BYTES, dtype=torch.uint8).pin_memory() for _ in range(self.RING)]
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
            image, label = crop_batch(self.pool, batch, self.transform, recs=self._recs[slot],
                                      label_dtype=self.label_dtype)
            ev = torch.cuda.Event()
            ev.record()
            self._events[slot] = ev
            yield {"image": image, "label": label}
