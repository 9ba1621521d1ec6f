"""Shared driver of all ``train_*.py`` command lines: Mean Teacher, UA-MT, ICT and deep co-training (``run_training``),
cross teaching, cross pseudo supervision and CNN-meets-ViT (``run_cross_teaching``), contrastive cross teaching
(``run_contrastive_cross``), triple view (``run_triple_view``), FixMatch (``run_fixmatch``) and adversarial network
training (``run_adversarial``).

Keeps what the reference scripts do around the hot loop (seeding, snapshot directory, ``log.txt``, the scalars, the
in-training validation, periodic checkpoints with the reference's file names, the two-stream "labeled first" batch
contract) and replaces the loop body by the ``step`` of a trainer of ``mis_hip.step``.  There is ONE loop (``run`` and its
core ``train_loop``); each ``run_*`` only describes its method as a ``Method`` and calls it.  Batches come from the dataset
under ``--root_path`` held resident in HBM (dataloaders/: two-stream sampler + one augmentation gather launch per batch) or,
when no dataset is there, from a synthetic two-stream source with the reference's shapes/dtypes.
"""
import dataclasses
import logging
import os
import random
import sys
import time
import types
import typing

import numpy as np
import torch


class SyntheticTwoStream:
    """Stands in for DataLoader(BaseDataSets / BraTS2019, TwoStreamBatchSampler): yields
    ``{'image': f32 [B,1,*patch], 'label': u8|i64 [B,*patch]}`` with the labeled samples FIRST
    (reference code/dataloaders/dataset.py:247-294).  Data are resident on the device."""

    def __init__(self, batch_size, patch_size, num_classes, label_dtype, seed, pool=4):
        g = torch.Generator(device="cuda").manual_seed(seed)
        self.batches = []
        for _ in range(pool):
            img = torch.rand((batch_size, 1) + tuple(patch_size), generator=g, device="cuda")
            lab = torch.randint(0, num_classes, (batch_size,) + tuple(patch_size), generator=g,
                                device="cuda").to(label_dtype)
            self.batches.append({"image": img, "label": lab})
        self.i = 0

    def __len__(self):
        return len(self.batches)

    def __iter__(self):
        for b in self.batches:
            yield b


def patients_to_slices(dataset, patiens_num):
    """Number of labeled slices for a number of labeled patients (reference train_mean_teacher_2D.py:106-116; like
    there, every dataset name without "ACDC" gets the Prostate table)."""
    if "ACDC" in dataset:
        ref_dict = {"3": 68, "7": 136, "14": 256, "21": 396, "28": 512, "35": 664, "140": 1312}
    else:
        ref_dict = {"2": 27, "4": 53, "8": 120, "12": 179, "16": 256, "21": 312, "42": 623}
    return ref_dict[str(patiens_num)]


def check_shards(n_labeled, n_unlabeled, labeled_bs, unlabeled_bs, world):
    """Every rank's labeled / unlabeled shard (``idxs[rank::world]``) must hold at least one batch, or
    ``TwoStreamBatchSampler`` asserts on SOME ranks only and the others hang in the first all-reduce.  The sizes are
    a pure function of (len, world), so every rank raises the same error together."""
    small = [(r, len(range(r, n_labeled, world)), len(range(r, n_unlabeled, world))) for r in range(world)]
    bad = [(r, l, u) for r, l, u in small if l < labeled_bs or u < unlabeled_bs]
    if bad:
        r, l, u = bad[0]
        raise RuntimeError(
            f"data-parallel shards too small for world={world}: rank {r} would get {l} labeled / {u} unlabeled "
            f"samples but a batch needs {labeled_bs} + {unlabeled_bs} (per GPU).  Use fewer GPUs, a smaller "
            f"--labeled_bs / --batch_size, or more labeled data (--labeled_num).")


def make_loader(args, label_dtype, rank, world=1, transform="random_generator"):
    """``transform`` (2-D): "random_generator" (the reference's RandomGenerator), "weak_strong" (its WeakStrongAugment: the
    batches are the weakly augmented ones, FixMatchTrainer makes the strong ones) or "weak" (its RandomGenerator_w: the
    nearest-neighbour resize alone, no rotation or flip).  The training batches: the dataset under ``--root_path`` resident in HBM with the reference's two-stream sampler
    and augmentation as one gather launch per batch (dataloaders/), or -- when no dataset is there (the list file
    ``train_slices.list`` / ``train.txt`` is missing) -- synthetic resident batches of the same shapes/dtypes."""
    three_d = len(args.patch_size) == 3
    listfile = os.path.join(args.root_path, "train.txt" if three_d else "train_slices.list")
    if not os.path.exists(listfile):
        return SyntheticTwoStream(args.batch_size, args.patch_size, args.num_classes, label_dtype,
                                  args.seed + 1000 * rank), "synthetic two-stream source (no dataset at %s)" % args.root_path
    if rank:                                   # data parallel: every rank draws its own batches / augmentations
        random.seed(args.seed + rank)
        np.random.seed(args.seed + rank)
    if three_d:
        from dataloaders.brats2019 import (BraTS2019, DeviceTwoStreamLoader3D, DeviceVolumePool, RandomRotFlipCrop,
                                           TwoStreamBatchSampler)
        db_train = BraTS2019(base_dir=args.root_path, split='train', num=None)
        # train_interpolation_consistency_training_3D.py:114-115 bounds the unlabeled pool by --total_labeled_num
        n_pool = min(len(db_train), getattr(args, "total_labeled_num", None) or len(db_train))
        check_shards(args.labeled_num, n_pool - args.labeled_num, args.labeled_bs,
                     args.batch_size - args.labeled_bs, world)
        labeled = list(range(0, args.labeled_num))[rank::world]           # train_mean_teacher_3D.py:109-112;
        unlabeled = list(range(args.labeled_num, n_pool))[rank::world]   # disjoint shard per rank (SURVEY s.8e)
        sampler = TwoStreamBatchSampler(labeled, unlabeled, args.batch_size, args.batch_size - args.labeled_bs)
        loader = DeviceTwoStreamLoader3D(DeviceVolumePool.from_dataset(db_train), sampler,
                                         RandomRotFlipCrop(args.patch_size), label_dtype=label_dtype)
    else:
        from dataloaders.dataset import (BaseDataSets, DeviceSlicePool, DeviceTwoStreamLoader, RandomGenerator,
                                         RandomGenerator_w, TwoStreamBatchSampler, WeakStrongAugment)
        transforms = {"random_generator": RandomGenerator, "weak_strong": WeakStrongAugment, "weak": RandomGenerator_w}
        if transform not in transforms:
            raise ValueError(f"unknown transform {transform!r}")
        db_train = BaseDataSets(base_dir=args.root_path, split="train", num=None)
        labeled_slice = patients_to_slices(args.root_path, args.labeled_num)   # train_mean_teacher_2D.py:172-180
        check_shards(labeled_slice, len(db_train) - labeled_slice, args.labeled_bs,
                     args.batch_size - args.labeled_bs, world)
        labeled = list(range(0, labeled_slice))[rank::world]
        unlabeled = list(range(labeled_slice, len(db_train)))[rank::world]
        sampler = TwoStreamBatchSampler(labeled, unlabeled, args.batch_size, args.batch_size - args.labeled_bs)
        loader = DeviceTwoStreamLoader(DeviceSlicePool.from_dataset(db_train), sampler,
                                       transforms[transform](args.patch_size))
    return loader, "%d cases of %s resident in HBM, %d labeled" % (len(db_train), args.root_path, len(labeled))


def setup_distributed():
    """One process per GPU (torchrun): returns (rank, world, local_rank); initialises RCCL if world > 1."""
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    torch.cuda.set_device(local_rank)
    if world > 1:
        # this rank's threads next to its GPU's PCIe root: its share of the cores of the device's NUMA node
        from . import dist as _dist
        local_world = int(os.environ.get("LOCAL_WORLD_SIZE", "0"))
        if local_world <= 0 and world <= torch.cuda.device_count():
            local_world = world                               # one node, launched without torchrun's LOCAL_WORLD_SIZE
        if local_world > 0:
            pin = _dist.pin_rank_to_numa(local_rank, local_world, _dist.device_bus_ids(min(local_world,
                                                                                             torch.cuda.device_count())))
        else:                                                 # several nodes and no LOCAL_WORLD_SIZE: the share is unknown
            pin = dict(applied=False, reason="LOCAL_WORLD_SIZE unset and WORLD_SIZE > local device count")
        logging.info("rank %d: CPU affinity %s", rank, pin)
    if world > 1 and not torch.distributed.is_initialized():
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        torch.distributed.init_process_group("nccl", device_id=torch.device("cuda", local_rank))
    return rank, world, local_rank


def broadcast_model_state(*models, src=0):
    """Every rank starts from (or resumes with) rank ``src``'s state: the flat parameter buffer AND the floating-point
    buffers (BatchNorm running statistics -- per-rank during training, rank 0's are the canonical ones a checkpoint holds)."""
    for m in models:
        if m is None:
            continue
        torch.distributed.broadcast(m.flat_param, src)
        bufs = [b for b in m.buffers() if b.is_floating_point() and b.numel()]
        if bufs:
            flat = torch.cat([b.detach().reshape(-1).float() for b in bufs])
            torch.distributed.broadcast(flat, src)
            off = 0
            with torch.no_grad():
                for b in bufs:
                    b.copy_(flat[off:off + b.numel()].view_as(b))
                    off += b.numel()


def _init_conv_weights(model, init_fn):
    """Shared body of the reference's ``kaiming_normal_init_weight`` / ``xavier_normal_init_weight``
    (train_cross_pseudo_supervision_3D.py:79-96, train_cross_pseudo_supervision_2D.py:85-102): ``init_fn`` on the
    weight of every nn.Conv2d / nn.Conv3d (NOT nn.ConvTranspose3d: ``isinstance(m, nn.Conv3d)`` is false for it),
    BatchNorm weight := 1, bias := 0.  Written in place through the flat-parameter views; draws from torch's global
    CPU generator in module order like the reference."""
    buffers = {n for n, _ in model.named_buffers()}
    transposed = getattr(model, "transposed_convs", ())
    for name, p in model.named_parameters():
        if p.dim() >= 4 and name.endswith(".weight") and name not in transposed:
            w = torch.empty(tuple(p.shape))
            init_fn(w)
            p.data.copy_(w)
        elif name.endswith(".weight") and p.dim() == 1 and name[:-len("weight")] + "running_mean" in buffers:
            p.data.fill_(1.0)
        elif name.endswith(".bias") and p.dim() == 1 and name[:-len("bias")] + "running_mean" in buffers:
            p.data.zero_()
    return model


def kaiming_normal_init_weight(model):
    return _init_conv_weights(model, torch.nn.init.kaiming_normal_)


def xavier_normal_init_weight(model):
    return _init_conv_weights(model, torch.nn.init.xavier_normal_)


def seed_everything(args):
    """reference train_mean_teacher_2D.py:316-326"""
    random.seed(args.seed)
    np.random.seed(args.seed)
    torch.manual_seed(args.seed)
    torch.cuda.manual_seed(args.seed)


class ScalarLog:
    """Tensorboard-free sink for the per-step scalars the reference sends to ``SummaryWriter.add_scalar``
    (train_mean_teacher_2D.py:239-250: info/lr, info/total_loss, info/loss_ce, info/loss_dice,
    info/consistency_loss, info/consistency_weight; the validation scalars :270-279): one CSV row
    ``iter_num,tag,value`` per call in ``<snapshot>/scalars.csv`` (tensorboardX is not in this image)."""

    def __init__(self, snapshot_path, enabled=True):
        self.f = open(os.path.join(snapshot_path, "scalars.csv"), "a") if enabled else None

    def add_scalar(self, tag, value, iter_num):
        if self.f is not None:
            self.f.write("%d,%s,%.9g\n" % (iter_num, tag, float(value)))

    def close(self):
        if self.f is not None:
            self.f.close()
            self.f = None


class Validator:
    """The in-training validation of the reference: every 200 iterations (``iter_num > 0 and iter_num % 200 == 0``)
    the model goes to eval mode and is scored on the validation split -- 2-D: ``val_2D.test_single_volume`` over
    ``BaseDataSets(split='val')`` (train_mean_teacher_2D.py:262-294), 3-D: ``val_3D.test_all_case(...,
    test_list='val.txt', stride_xy=64, stride_z=64)`` (train_mean_teacher_3D.py:201-222) -- and a new best mean Dice
    writes ``<prefix>iter_{n}_dice_{d}.pth`` and ``{model}_best_<name>.pth``.  Data-parallel runs (the reference is
    single-GPU) shard the validation cases over the ranks (``cases[rank::world]``) and all-reduce the metric sums: no
    rank waits in the next step's gradient all-reduce for a whole validation pass on rank 0 (RCCL's watchdog would
    abort a long 3-D one).  Every rank holds identical weights; the BatchNorm running statistics -- per-rank, there is
    no SyncBN -- are taken from rank 0 for the scoring, as the checkpoint is, and every rank's OWN running statistics are
    put back afterwards: validation never changes the training state, the ranks' running statistics evolve independently for the
    whole run (standard DDP without SyncBN) and rank 0 is canonical -- its buffers are what checkpoints hold and what
    ``resume`` broadcasts (train_common.broadcast_model_state).  Scalars, logs and checkpoints are rank 0's.  When the validation list file is missing (the synthetic runs) nothing is scored and ``finish`` writes
    the final weights under the best-model name, so that the inference CLIs always find their checkpoint."""

    def __init__(self, args, snapshot_path, scalars=None, rank=0, world=1, process_group=None, save=None):
        """``save(model, path)`` writes a new best model; the default is the bare ``state_dict`` of the reference."""
        self.args, self.snapshot_path, self.scalars = args, snapshot_path, scalars
        self.save = save or (lambda model, path: torch.save(model.state_dict(), path))
        self.rank, self.world = rank, world
        self.pg = process_group          # the trainer's group: validation collectives must run where the gradients do
        self.three_d = len(args.patch_size) == 3
        self.best = {}
        self.db_val = None
        listfile = os.path.join(args.root_path, "val.txt" if self.three_d else "val.list")
        self.available = os.path.exists(listfile)
        if self.available and not self.three_d:
            from dataloaders.dataset import BaseDataSets
            self.db_val = BaseDataSets(base_dir=args.root_path, split="val")

    def score(self, model):
        """(mean Dice, mean HD95, per-class [[dice, hd95], ...]) of ``model`` on the validation split."""
        args = self.args
        saved = None
        if self.world > 1:
            # score with rank 0's BatchNorm running statistics on every rank: ONE broadcast of the floating-point buffers
            # packed into a flat tensor (dozens of tiny collectives per model before).  The rank's own statistics are put
            # back after the scoring -- validation must not change the training state (per-rank running statistics, no
            # SyncBN, are what the reference's single-GPU semantics give every rank).
            bufs = [b for b in model.buffers() if b.is_floating_point() and b.numel()]
            if bufs:
                saved = [b.detach().clone() for b in bufs]
                flat = torch.cat([b.detach().reshape(-1).float() for b in bufs])
                src = torch.distributed.get_global_rank(self.pg, 0) if self.pg is not None else 0
                torch.distributed.broadcast(flat, src, group=self.pg)
                off = 0
                with torch.no_grad():
                    for b in bufs:
                        b.copy_(flat[off:off + b.numel()].view_as(b))
                        off += b.numel()
        err = None
        try:
            total, count = self._score_shard(model)
        except Exception as e:       # keep the collective below symmetric: the other ranks must not wait for this one
            if self.world <= 1:
                raise
            err, total, count = e, np.zeros((args.num_classes - 1, 2)), 0
        finally:
            if saved is not None:
                with torch.no_grad():
                    for b, v in zip(bufs, saved):
                        b.copy_(v)
        m = self._reduce(total, count, failed=err is not None)
        if err is not None:
            raise err
        return float(np.mean(m, axis=0)[0]), float(np.mean(m, axis=0)[1]), m

    def _score_shard(self, model):
        args = self.args
        if self.three_d:
            from val_3D import test_all_case
            total, count = test_all_case(model, args.root_path, test_list="val.txt", num_classes=args.num_classes,
                                         patch_size=args.patch_size, stride_xy=64, stride_z=64,
                                         shard=(self.rank, self.world))
        else:
            from val_2D import test_single_volume
            total, count = np.zeros((args.num_classes - 1, 2)), 0
            for i in range(self.rank, len(self.db_val), self.world):
                s = self.db_val[i]
                image = torch.from_numpy(np.asarray(s["image"])).unsqueeze(0)
                label = torch.from_numpy(np.asarray(s["label"])).unsqueeze(0)
                total = total + np.array(test_single_volume(image, label, model, classes=args.num_classes,
                                                            patch_size=args.patch_size), dtype=np.float64)
                count += 1
        return total, count

    def _reduce(self, total, count, failed=False):
        """Mean over all ranks' cases: all-reduce (sum) of the metric sums, the case count and an error flag -- a rank whose
        shard raised still takes part, and EVERY rank then fails (instead of the others blocking in this all-reduce until
        the process group's timeout)."""
        if self.world > 1:
            t = torch.tensor(np.concatenate([np.asarray(total, dtype=np.float64).ravel(), [float(count), float(failed)]]),
                             dtype=torch.float64,
                             device="cuda" if torch.distributed.get_backend(self.pg) == "nccl" else "cpu")
            torch.distributed.all_reduce(t, group=self.pg)
            t = t.cpu().numpy()
            if t[-1] > 0 and not failed:
                raise RuntimeError(f"validation failed on {int(t[-1])} other rank(s); see their logs")
            total, count = t[:-2].reshape(np.shape(total)), t[-2]
        return np.asarray(total, dtype=np.float64) / max(count, 1)

    def __call__(self, iter_num, models):
        """``models``: list of (tag, file prefix, best-file suffix, module), e.g. ('', '', 'best_model', model) or
        ('model1_', 'model1_', 'best_model1', model1)."""
        if not self.available or iter_num <= 0 or iter_num % 200:
            return
        for tag, prefix, best_name, model in models:
            was_training = model.training
            model.eval()
            perf, hd95, m = self.score(model)
            model.train(was_training)
            if self.rank != 0:
                continue
            if self.scalars is not None:
                for c in range(m.shape[0]):
                    self.scalars.add_scalar('info/%sval_%d_dice' % (tag, c + 1), m[c, 0], iter_num)
                    self.scalars.add_scalar('info/%sval_%d_hd95' % (tag, c + 1), m[c, 1], iter_num)
                self.scalars.add_scalar('info/%sval_mean_dice' % tag, perf, iter_num)
                self.scalars.add_scalar('info/%sval_mean_hd95' % tag, hd95, iter_num)
            if perf > self.best.get(best_name, 0.0):
                self.best[best_name] = perf
                self.save(model, os.path.join(
                    self.snapshot_path, '%siter_%d_dice_%s.pth' % (prefix, iter_num, round(perf, 4))))
                self.save(model, os.path.join(self.snapshot_path, '%s_%s.pth' % (self.args.model, best_name)))
            if self.three_d:      # train_mean_teacher_3D.py:221-222
                logging.info('iteration %d : %sdice_score : %f %shd95 : %f' % (iter_num, tag, perf, tag, hd95))
            else:                 # train_mean_teacher_2D.py:292-293
                logging.info('iteration %d : %smean_dice : %f %smean_hd95 : %f' % (iter_num, tag, perf, tag, hd95))

    def finish(self, models):
        if self.rank != 0:
            return
        for tag, prefix, best_name, model in models:
            path = os.path.join(self.snapshot_path, '%s_%s.pth' % (self.args.model, best_name))
            if not os.path.exists(path):
                torch.save(model.state_dict(), path)
                logging.info("no validation score was recorded (%s): final weights saved as %s" %
                             ("no validation list under %s" % self.args.root_path if not self.available
                              else "fewer than 200 iterations or Dice 0", path))


def open_snapshot(args, rank, fmt="../model/{}_{}_labeled/{}"):
    """``fmt``: the snapshot directory pattern of the reference script being mirrored (it differs between scripts:
    train_mean_teacher_2D.py:328 has the ``_labeled`` suffix, train_mean_teacher_3D.py:252 and the cross-teaching /
    CPS scripts do not)."""
    snapshot_path = fmt.format(args.exp, args.labeled_num, args.model)
    if rank == 0:
        os.makedirs(snapshot_path, exist_ok=True)
        logging.basicConfig(filename=snapshot_path + "/log.txt", level=logging.INFO,
                            format='[%(asctime)s.%(msecs)03d] %(message)s', datefmt='%H:%M:%S', force=True)
        logging.getLogger().addHandler(logging.StreamHandler(sys.stdout))
        logging.info(str(args))
    return snapshot_path


def save_checkpoint(epoch, model, trainer, loss, path):
    """A checkpoint in the shape of the reference's ``util.save_checkpoint`` (code/utils/util.py:113-123):
    ``{"epoch", "state_dict", "optimizer_state_dict", "loss"}``.  ``state_dict`` is ``model.state_dict()``.
    ``optimizer_state_dict`` is NOT a ``torch.optim`` state dict: the optimizer here is the fused SGD kernel, whose state
    is the flat momentum buffer and the iteration (the learning rate follows from it): ``{"momentum_buffer", "iter_num"}``."""
    torch.save({"epoch": int(epoch), "state_dict": model.state_dict(),
                "optimizer_state_dict": {"momentum_buffer": trainer.momentum_buf.detach().cpu(),
                                         "iter_num": int(trainer.iter_num)},
                "loss": torch.as_tensor(float(loss))}, path)


def load_checkpoint(path, model):
    """(epoch, iter_num, momentum buffer, loss) of a ``save_checkpoint`` file; the weights go into ``model``."""
    ck = torch.load(path, map_location="cpu")
    model.load_state_dict(ck["state_dict"])
    opt = ck["optimizer_state_dict"]
    return int(ck["epoch"]), int(opt["iter_num"]), opt["momentum_buffer"], float(ck["loss"])


def newest_checkpoint(snapshot_path):
    """``model_iter_<n>.pth`` / ``model_iter_<n>_dice_<d>.pth`` with the largest n under ``snapshot_path`` (the search of
    train_Fixmatch_CNN_2D.py:196-206), or None."""
    best = None
    if os.path.isdir(snapshot_path):
        for name in os.listdir(snapshot_path):
            if name.startswith("model_iter_") and name.endswith(".pth"):
                try:
                    n = int(os.path.splitext(name)[0].split("_")[2])
                except ValueError:
                    continue
                if best is None or n > best[0]:
                    best = (n, os.path.join(snapshot_path, name))
    return best[1] if best else None


@dataclasses.dataclass
class Method:
    """What one training method changes in ``run``; everything not named here is the same for all of them.

    ``nets`` lists the networks as ``(stem, factory)``, the students first and the ``ema`` EMA copies (parameters detached)
    last; they are built in this order.  The stem names everything a network leaves behind: ``''`` | ``'model_'`` |
    ``'model1_'`` | ``'ema_model_'`` gives the validation tags ``info/<stem>val_*``, the files ``<stem>iter_<n>.pth``,
    ``<stem>iter_<n>_dice_<d>.pth`` and ``{model}_best_<name>.pth`` and the log line ``save <name> to``, where the name is
    the stem without its underscore (``model`` for the empty stem).  ``make_trainer(models, ctx)`` gets all networks and
    ``ctx.rank``, ``ctx.world``, ``ctx.iter_num`` (non-zero on resume) and, with ``loader_first``, ``ctx.iters_per_epoch``.
    ``scalars(s, lr_)`` returns the ``(tag, value)`` rows of an iteration and ``log_line(iter_num, s)`` its log line: ``s`` is
    ``trainer.losses()`` and ``lr_`` the poly rate the step ran with, which is the one the reference scripts log."""
    nets: list
    make_trainer: typing.Callable
    scalars: typing.Callable
    log_line: typing.Callable
    snapshot_fmt: str                       # the snapshot directory pattern of the script being mirrored (open_snapshot)
    label_dtype: torch.dtype = torch.uint8
    ema: int = 0
    init_fns: tuple = ()                    # on the first students, once ALL students are built and before an EMA copy is
    transform: str = "random_generator"     # make_loader's 2-D batch transform
    loader_first: bool = False              # the trainer needs len(loader): the loader is built before it, not after it
    validated: tuple = (0,)                 # indices into nets: scored every 200 iterations
    saved: tuple = (0,)                     # indices into nets: written every 3000 iterations
    last_model: bool = False                # ``{model}_last_model.pth`` at the end of the run
    checkpoints: bool = False               # train_Fixmatch_CNN_2D.py: files are ``save_checkpoint`` dictionaries; ``--load``
    extra_files: typing.Callable = None     # (trainer, snapshot_path, iter_num): more periodic files, beside those of ``saved``


def _name(stem):
    return stem[:-1] or "model"


def _val_models(method, models):
    """The Validator's (tag, file prefix, best-file suffix, module) of every validated network."""
    return [(method.nets[i][0], method.nets[i][0], "best_" + _name(method.nets[i][0]), models[i]) for i in method.validated]


def train_loop(args, method, rank, models, trainer, loader, validator, scalars, progress):
    """The one epoch / batch loop: ``trainer.step``, the scalars and the log line on rank 0, validation on every rank, the
    periodic files every 3000 iterations, until ``args.max_iterations``.  Starts at ``progress.iter_num`` / ``.epoch`` and
    keeps ``progress`` (with ``.losses``, those of the last logged iteration) current.  Touches no device itself: the only
    host read is ``trainer.losses()``, once per logged iteration and once more per periodic file of a ``checkpoints``
    method.  Returns the number of iterations done."""
    val_models = _val_models(method, models)
    done = 0
    for epoch in range(progress.epoch, args.max_iterations // len(loader) + 1):
        progress.epoch = epoch
        for sampled_batch in loader:
            # lr_ as the reference logs it: computed BEFORE iter_num += 1 and logged under the incremented iter_num
            # (train_mean_teacher_2D.py:234, train_tripleview_2D(demo).py:346-347, train_Fixmatch_CNN_2D.py:297); a run
            # that starts below max_iterations leaves the loop before this count can pass it, so the base stays >= 0
            lr_ = args.base_lr * (1.0 - progress.iter_num / args.max_iterations) ** 0.9
            trainer.step(sampled_batch["image"], sampled_batch["label"])
            done += 1
            progress.iter_num += 1
            iter_num = progress.iter_num
            if rank == 0:
                s = progress.losses = trainer.losses()      # the only device->host read of the step
                for tag, value in method.scalars(s, lr_):
                    scalars.add_scalar(tag, value, iter_num)
                logging.info(method.log_line(iter_num, s))
            validator(iter_num, val_models)      # every rank: the validation cases are sharded over the ranks
            if rank == 0 and iter_num % 3000 == 0:
                for i in method.saved:
                    stem = method.nets[i][0]
                    path = os.path.join(validator.snapshot_path, '%siter_%d.pth' % (stem, iter_num))
                    if method.checkpoints:
                        save_checkpoint(epoch, models[i], trainer, trainer.losses()["loss"], path)
                    else:
                        torch.save(models[i].state_dict(), path)
                    logging.info("save %s to %s" % (_name(stem), path))
                if method.extra_files is not None:
                    method.extra_files(trainer, validator.snapshot_path, iter_num)
            if iter_num >= args.max_iterations:
                return done
    return done


def run(args, method):
    """A whole training run of ``method`` (a ``Method``) for the parsed command line ``args``: ranks, seed and snapshot
    directory; the networks, every rank starting from rank 0's; trainer and loader; ``train_loop``; the final files."""
    rank, world, _ = setup_distributed()
    seed_everything(args)
    snapshot_path = open_snapshot(args, rank, method.snapshot_fmt)
    students = len(method.nets) - method.ema
    models = [make() for _, make in method.nets[:students]]
    for init, m in zip(method.init_fns, models):     # e.g. kaiming_normal / xavier_normal of the CPS scripts
        init(m)
    models += [make() for _, make in method.nets[students:]]
    for m in models[students:]:
        for p in m.parameters():           # create_model(ema=True): teacher params are detached
            p.detach_()
    progress = types.SimpleNamespace(iter_num=0, epoch=0, losses={})
    momentum = None
    if method.checkpoints and args.load:   # resume from the newest model_iter_*.pth: weights, momentum, iteration, epoch
        path = newest_checkpoint(snapshot_path)
        if path is None:
            logging.warning("no model_iter_*.pth under %s: using a new model" % snapshot_path)
        else:
            progress.epoch, progress.iter_num, momentum, _ = load_checkpoint(path, models[0])
            logging.info("Models restored from iteration %d (%s)" % (progress.iter_num, path))
    start_epoch = progress.epoch
    if world > 1:                          # every rank starts from rank 0's weights and running statistics
        broadcast_model_state(*models)
    for m in models:
        m.train()
    ctx = types.SimpleNamespace(rank=rank, world=world, iter_num=progress.iter_num, iters_per_epoch=None)
    if method.loader_first:
        loader, source = make_loader(args, method.label_dtype, rank, world, transform=method.transform)
        ctx.iters_per_epoch = len(loader)
    trainer = method.make_trainer(models, ctx)
    if momentum is not None:
        trainer.momentum_buf.copy_(momentum)
    if not method.loader_first:
        loader, source = make_loader(args, method.label_dtype, rank, world, transform=method.transform)
    if rank == 0:
        logging.info("{} iterations per epoch ({})".format(len(loader), source))
    scalars = ScalarLog(snapshot_path, enabled=(rank == 0))
    save = None
    if method.checkpoints:                 # train_Fixmatch_CNN_2D.py:346-354: a new best model is a checkpoint too
        save = lambda model, path: save_checkpoint(progress.epoch, model, trainer, progress.losses.get("loss", 0.0), path)
    validator = Validator(args, snapshot_path, scalars, rank, world, process_group=trainer.pg, save=save)
    t0 = time.time()
    done = train_loop(args, method, rank, models, trainer, loader, validator, scalars, progress)
    torch.cuda.synchronize()
    if rank == 0:
        dt = time.time() - t0
        logging.info("%d iterations in %.2f s (%.1f samples/s over %d GPU(s))" %
                     (done, dt, done * args.batch_size * world / max(dt, 1e-9), world))
        if method.last_model:
            torch.save(models[0].state_dict(), os.path.join(snapshot_path, '{}_last_model.pth'.format(args.model)))
        if not method.checkpoints:
            validator.finish(_val_models(method, models))
        else:                              # no validation score was recorded: the inference CLI still finds its file
            path = os.path.join(snapshot_path, '{}_best_model.pth'.format(args.model))
            if not os.path.exists(path):
                save_checkpoint(start_epoch, models[0], trainer, trainer.losses()["loss"], path)
                logging.info("no validation score was recorded: final weights saved as %s" % path)
        scalars.close()
    if world > 1:
        torch.distributed.destroy_process_group()
    return "Training Finished!"


def _common_kw(args, rank):
    """The keyword arguments every trainer class takes."""
    return dict(labeled_bs=args.labeled_bs, num_classes=args.num_classes, base_lr=args.base_lr,
                max_iterations=args.max_iterations, consistency=args.consistency,
                consistency_rampup=args.consistency_rampup, seed=args.seed + rank)


def _tagged_losses(s, lr_):
    """Every entry of ``losses()`` under ``loss/<key>``, but the consistency weight and (ContrastiveCrossTrainer has it)
    the learning rate under the reference's own tags (train_cross_teaching_between_cnn_transformer_2D.py:263-270,
    train_Contrastive_Cross_CNN_2D.py:286-292)."""
    own = {"lr": "lr", "consistency_weight": "consistency_weight/consistency_weight"}
    return [(own.get(k, "loss/" + k), v) for k, v in s.items()]


def run_training(args, make_model, *, label_dtype, cons_start_iter, save_ema, trainer_cls=None,
                 snapshot_fmt="../model/{}_{}_labeled/{}", trainer_kw=None, single_model=False):
    """train_mean_teacher_2D.py:196-312 / train_mean_teacher_3D.py:128-230 (and, with ``trainer_cls=UAMTTrainer``,
    train_uncertainty_aware_mean_teacher_{2D,3D}.py; with ``trainer_cls=ICTTrainer`` and ``trainer_kw=dict(ict_alpha=...)``,
    train_interpolation_consistency_training_{2D,3D,2D_ViT}.py).  ``trainer_kw``: extra keyword arguments of the trainer
    class.  ``single_model=True``: no EMA teacher is built and the trainer class takes the one network alone
    (``trainer_cls=DeepCoTrainingTrainer``: train_deep_co_training_2D{,_ViT}.py:116-237)."""
    from .step import MeanTeacherTrainer

    def make_trainer(models, ctx):
        kw = dict(_common_kw(args, ctx.rank), **(trainer_kw or {}))
        if not single_model:
            kw.update(ema_decay=args.ema_decay, cons_start_iter=cons_start_iter)
        if trainer_cls is None:
            # captured replay of a step that contains an RCCL collective is not verified on hardware: --hip_graph is
            # honoured for single-GPU runs only
            kw.update(use_graph=bool(getattr(args, "hip_graph", 0)) and ctx.world == 1)
        if ctx.rank == 0 and getattr(args, "hip_graph", 0) and ctx.world > 1:
            logging.info("--hip_graph ignored for world_size %d (single-GPU only)" % ctx.world)
        return (trainer_cls or MeanTeacherTrainer)(*models, **kw)

    # all scalars of train_mean_teacher_2D.py:239-245
    return run(args, Method(
        nets=[('', make_model)] if single_model else [('', make_model), ('ema_model_', make_model)],
        ema=0 if single_model else 1, make_trainer=make_trainer, saved=(0, 1) if save_ema else (0,), last_model=True,
        scalars=lambda s, lr_: [('info/lr', lr_), ('info/total_loss', s["loss"]), ('info/loss_ce', s["loss_ce"]),
                                ('info/loss_dice', s["loss_dice"]), ('info/consistency_loss', s["consistency_loss"]),
                                ('info/consistency_weight', s["consistency_weight"])],
        log_line=lambda it, s: 'iteration %d : loss : %f, loss_ce: %f, loss_dice: %f' % (it, s["loss"], s["loss_ce"],
                                                                                        s["loss_dice"]),
        snapshot_fmt=snapshot_fmt, label_dtype=label_dtype))


def run_cross_teaching(args, make_model1, make_model2, label_dtype=torch.uint8, pseudo_ce=False, make_ema=None,
                       snapshot_fmt="../model/{}_{}/{}", init_fns=()):
    """train_cross_teaching_between_cnn_transformer_2D.py:208-300 (two students, no teacher); with ``pseudo_ce=True``
    train_cross_pseudo_supervision_{2D,3D}.py (CE pseudo-supervision); with ``make_ema`` (the EMA teacher of model2, which
    is validated too: :441-468) train_cnn_meet_vit_2D.py:285-352."""
    from .step import CnnMeetVitTrainer, CrossTeachingTrainer
    nets = [('model1_', make_model1), ('model2_', make_model2)]
    if make_ema is not None:
        nets.append(('ema_model_', make_ema))
        make_trainer = lambda models, ctx: CnnMeetVitTrainer(*models, ema_decay=args.ema_decay, **_common_kw(args, ctx.rank))
    else:
        make_trainer = lambda models, ctx: CrossTeachingTrainer(*models, pseudo_ce=pseudo_ce, **_common_kw(args, ctx.rank))
    return run(args, Method(
        nets=nets, ema=len(nets) - 2, init_fns=init_fns, make_trainer=make_trainer, validated=tuple(range(len(nets))),
        saved=(0, 1), scalars=_tagged_losses,
        log_line=lambda it, s: 'iteration %d : model1 loss : %f model2 loss : %f' % (it, s["model1_loss"], s["model2_loss"]),
        snapshot_fmt=snapshot_fmt, label_dtype=label_dtype))


def run_contrastive_cross(args, make_model1, make_model2, label_dtype=torch.uint8,
                          snapshot_fmt="../model/{}_{}_labeled/{}"):
    """train_Contrastive_Cross_CNN_2D.py:196-408 (and its _CNN_ViT_ twin): two students around ``ContrastiveCrossTrainer``
    with the four frozen heads of ``net_factory("classifier" | "projector")``, the resize-only weak loader (the strong
    loader's batch is never read by the loss: it is not built), the script's scalars (:286-292) and its log line (:294).
    The trainer needs the loader's length (the script's consistency ramp counts epochs), so the loader comes first."""
    from networks.net_factory import net_factory
    from .step import ContrastiveCrossTrainer

    def make_trainer(models, ctx):
        heads = [net_factory(k).train() for k in ("classifier", "classifier", "projector", "projector")]     # :139-142
        return ContrastiveCrossTrainer(*models, *heads, iters_per_epoch=ctx.iters_per_epoch, **_common_kw(args, ctx.rank))

    return run(args, Method(
        nets=[('model1_', make_model1), ('model2_', make_model2)], make_trainer=make_trainer, loader_first=True,
        transform="weak", validated=(0, 1), saved=(0, 1), scalars=_tagged_losses,
        log_line=lambda it, s: ('itr %d, loss %0.2f, m1 loss %0.2f, m2 loss %0.2f, con_loss %0.2f,c_loss_l %0.2f,'
                                'c_loss_u %0.2f, lr %f' % (it, s["loss"], s["model1_loss"], s["model2_loss"], s["con_loss"],
                                                          s["c_loss_l"], s["c_loss_u"], s["lr"])),
        snapshot_fmt=snapshot_fmt, label_dtype=label_dtype))


def run_triple_view(args, make_models, label_dtype=torch.uint8, snapshot_fmt="../model/{}_{}/{}"):
    """train_tripleview_2D(demo).py:283-491: three students (``make_models``: three factories), no teacher.  The same
    scalars and log line as the reference (:356-362), all three models validated every 200 iterations (:379-471), the
    periodic checkpoints every 3000 (:473-484)."""
    from .step import TripleViewTrainer, triple_split
    triple_split(args.batch_size, args.labeled_bs)
    return run(args, Method(
        nets=list(zip(('model1_', 'model2_', 'model3_'), make_models)), validated=(0, 1, 2), saved=(0, 1, 2),
        make_trainer=lambda models, ctx: TripleViewTrainer(*models, **_common_kw(args, ctx.rank)),
        scalars=lambda s, lr_: [('lr', lr_), ('consistency_weight/consistency_weight', s["consistency_weight"]),
                                ('loss/model1_loss', s["model1_loss"]), ('loss/model2_loss', s["model2_loss"]),
                                ('loss/model3_loss', s["model3_loss"])],
        log_line=lambda it, s: 'iteration %d : model1 loss : %f model2 loss : %f : model3 loss: %f' % (
            it, s["model1_loss"], s["model2_loss"], s["model3_loss"]),
        snapshot_fmt=snapshot_fmt, label_dtype=label_dtype))


def run_fixmatch(args, make_model, label_dtype=torch.uint8, snapshot_fmt="../model/{}_{}/{}"):
    """train_Fixmatch_CNN_2D.py:243-372: one network and the EMA copy the reference keeps updated, ``FixMatchTrainer.step``
    on the weakly augmented batches (the strong ones are made inside the step), the reference's scalar tags (:303-305,
    :328-344) and log line, ``model_iter_{n}_dice_{d}.pth`` / ``{model}_best_model.pth`` and the periodic
    ``model_iter_{n}.pth``, all in the ``util.save_checkpoint`` shape.  ``--load`` resumes from the newest
    ``model_iter_*.pth``: weights, momentum buffer, iteration and epoch."""
    from .step import FixMatchTrainer, fixmatch_split
    fixmatch_split(args.batch_size, args.labeled_bs)
    return run(args, Method(
        nets=[('model_', make_model), ('ema_model_', make_model)], ema=1, transform="weak_strong", checkpoints=True,
        make_trainer=lambda models, ctx: FixMatchTrainer(*models, ema_decay=args.ema_decay, conf_thresh=args.conf_thresh,
                                                         iter_num=ctx.iter_num, **_common_kw(args, ctx.rank)),
        scalars=lambda s, lr_: [('lr', lr_), ('consistency_weight/consistency_weight', s["consistency_weight"]),
                                ('loss/model_loss', s["loss"])],
        log_line=lambda it, s: 'iteration %d : model loss : %f' % (it, s["loss"]),
        snapshot_fmt=snapshot_fmt, label_dtype=label_dtype))


def run_adversarial(args, make_model, make_dan, label_dtype=torch.int64, snapshot_fmt="../model/{}_{}/{}"):
    """train_adversarial_network_3D.py:84-238: the segmenter and the discriminator around ``AdversarialTrainer``, the
    script's scalars (:177-184) and log line (:186-188), the segmenter validated every 200 iterations and written every
    3000 as the reference does (``iter_<n>.pth``, ``{model}_best_model.pth``).  Beside every ``iter_<n>.pth`` goes
    ``DAN_iter_<n>.pth``: the discriminator's state_dict, Adam's two moment buffers and its step count
    (``AdversarialTrainer.dan_checkpoint``)."""
    from .step import AdversarialTrainer

    def extra_files(trainer, snapshot_path, iter_num):
        path = os.path.join(snapshot_path, 'DAN_iter_%d.pth' % iter_num)
        torch.save(trainer.dan_checkpoint(), path)
        logging.info("save DAN to %s" % path)

    return run(args, Method(
        nets=[('', make_model), ('DAN_', make_dan)], extra_files=extra_files,
        make_trainer=lambda models, ctx: AdversarialTrainer(*models, dan_lr=args.DAN_lr, **_common_kw(args, ctx.rank)),
        scalars=lambda s, lr_: [('info/lr', lr_), ('info/total_loss', s["loss"]), ('info/loss_ce', s["loss_ce"]),
                                ('info/loss_dice', s["loss_dice"]), ('info/consistency_loss', s["consistency_loss"]),
                                ('info/consistency_weight', s["consistency_weight"]), ('info/DAN_loss', s["DAN_loss"])],
        log_line=lambda it, s: 'iteration %d : loss : %f, loss_ce: %f, loss_dice: %f' % (it, s["loss"], s["loss_ce"],
                                                                                        s["loss_dice"]),
        snapshot_fmt=snapshot_fmt, label_dtype=label_dtype))
