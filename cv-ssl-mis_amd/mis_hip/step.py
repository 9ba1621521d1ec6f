"""The training steps, each one fused device-side sequence replacing a loop body of the reference.

Ten methods share one skeleton (``_Step``); DESIGN.md has a section per method:

    MeanTeacherTrainer      student + EMA teacher on the noised unlabeled half (code/train_mean_teacher_{2D,3D}.py)
    UAMTTrainer             + T = 8 MC-dropout teacher passes, the entropy of their mean masks the consistency term
    ICTTrainer              student on mixed unlabeled samples, pulled towards the mix of two teacher predictions
    DeepCoTrainingTrainer   one network, a pass on the batch and one on its rotated unlabeled half
    FixMatchTrainer         one network, a pass on the weak batch and one on its colour-jittered copy; pseudo + complementary labels
    CrossTeachingTrainer    two students teach each other through arg-max pseudo labels (``pseudo_ce``: CPS)
    ContrastiveCrossTrainer cross teaching + two pixel-wise contrastive terms through frozen projector / classifier heads
    CnnMeetVitTrainer       cross teaching + an EMA teacher of the second student
    TripleViewTrainer       three students, each taught by the arg-max pseudo labels of both others; one joint loss tail
    AdversarialTrainer      a 3-D student and a discriminator (SGD / Adam), two phases per step (code/train_adversarial_network_3D.py)

The skeleton of a step:

    inputs (noise / mix / rotation) -> forwards, the independent ones beside each other on a side stream (``_beside``)
    -> one fused loss tail per student (losses + dlogits) -> backward(s) -> [RCCL all-reduce of the flat gradient bucket(s)]
    -> fused SGD + EMA per student, then the poly-LR / EMA-alpha / consistency-weight schedule advanced on the device
    (``_finish_step``)

A trainer's ``_run`` is what is particular to its method: which inputs it builds, which forwards run, which tail is called.
Nothing in the sequence allocates or synchronises with the host: scalars stay in a small device buffer (``trainer.out``,
or ``out1`` / ``out2`` (/ ``out3``) with two (three) students) that the caller reads when it wants to log (the reference forces >= 3 + C host
syncs per step).  The RNG offset, learning rate, EMA alpha and the consistency weight live in a
device-resident ``MisStepState``, so a recorded step stays correct when it is replayed: from a launch tape (``_TapedStep``,
every trainer but UA-MT), or, for the Mean-Teacher step, from a captured hipGraph (``use_graph=True``).
"""
import os
import random

import torch

from . import dist, ops
from . import lib as _lib

# teacher forward (cross teaching: the second student) on a side stream, see _Step._beside: bit-identical training, the second
# network's launches fill the CUs the first one's launch tails and small deep layers leave idle (MIS_TWO_STREAM=0: off)
TWO_STREAM = os.environ.get("MIS_TWO_STREAM", "1") != "0"
# the step as a launch tape (lib.LaunchTape): after two eager steps the trainer records one step's launches and replays them --
# one ctypes call per launch instead of the Python op graph (host enqueue 8.6 -> ~2 ms of a 20 ms SwinUnet step; a captured
# hipGraph costs the host MORE than the eager step on this stack).  MIS_STEP_TAPE=0: eager.  Bit-identical training.
STEP_TAPE = os.environ.get("MIS_STEP_TAPE", "1") != "0"
# data parallel: issue the all-reduce of finished gradient buckets while the backward is still running
# (dist.GradBucketer); MIS_GRAD_OVERLAP=0 falls back to one blocking all-reduce after the backward
GRAD_OVERLAP = os.environ.get("MIS_GRAD_OVERLAP", "1") != "0"


def backward_and_sync(model, pg, bucketer=None):
    """Student backward + the step's only exchange: the all-reduce (sum) of the flat gradient bucket.  Returns the
    1/world scale the optimizer kernel folds in.  With a bucketer the finished buckets travel during the backward."""
    if bucketer is None:
        model.backward_raw()
        return _lib.tape_call(dist.sync_gradients, model.flat_grad, pg)
    _lib.tape_call(bucketer.begin)
    model.backward_raw(on_progress=bucketer.advance)
    return _lib.tape_call(bucketer.finish)


def make_bucketer(model, pg, defer_tail=False):
    """MIS_FORCE_BUCKETER=1: the bucketer also for a single-rank group (tests / scripts/ddp_overhead.py run the RCCL
    stream machinery on one GPU)."""
    on = dist.world_size(pg) > 1 or (os.environ.get("MIS_FORCE_BUCKETER", "0") == "1" and dist.initialized())
    return dist.GradBucketer(model.flat_grad, pg, defer_tail=defer_tail) if (GRAD_OVERLAP and on) else None


class _TapedStep:
    """Mixin: ``_tape_step(run, tensors)`` runs ``run(*static)`` eagerly twice (plans, scratch buffers and lazily built job
    tables settle), records the third run as a lib.LaunchTape and replays it from then on.  ``tensors`` are the step's inputs:
    the recording sees static copies (or the caller's own tensors when they are the same storage every step, as in bench.py)."""

    _tape = None
    _tape_warm = 0
    _tape_static = None
    TAPE_WARMUP = 2

    def _tape_step(self, run, tensors):
        if self._tape is None:
            if self._tape_warm < self.TAPE_WARMUP:
                self._tape_warm += 1
                run(*tensors)
                return
            self._tape_static = tuple(t.clone() for t in tensors)
            tape = _lib.LaunchTape()
            with tape.recording():
                run(*self._tape_static)
            self._tape = tape
            return
        for t, st in zip(tensors, self._tape_static):
            if t.shape != st.shape or t.dtype != st.dtype:
                raise RuntimeError("the taped step was recorded for inputs of another shape; construct the trainer with "
                                   "use_tape=False (MIS_STEP_TAPE=0) for varying batch geometry")
            st.copy_(t)
        self._tape.replay()


class _Step(_TapedStep):
    """What every training step here is made of; a trainer adds its constructor signature, ``TRAIN_MODE`` (the message for a
    network found in eval mode) and ``_run(volume, label, *inject)``, the step in its eager form -- also what is recorded."""

    TRAIN_MODE = None
    _side = None            # the side stream of _beside, created on first use
    _ema_in = None          # the teacher's noised input (_noised)

    def _setup(self, students, teachers, rng_streams, *, labeled_bs, num_classes, base_lr, max_iterations, consistency,
               consistency_rampup, seed, iter_num, momentum, weight_decay, process_group, use_tape, ema_decay=0.0,
               cons_start_iter=0, lr_post_increment=False):
        """Step state and schedule, the networks bound to them, one momentum and one scalar buffer per student.
        ``rng_streams``: the Philox dropout sub-stream of each network (students, then teachers): seed-reproducible, distinct."""
        self._students, self._nets = tuple(students), tuple(students) + tuple(teachers)
        self.labeled_bs, self.num_classes = labeled_bs, num_classes
        # the keyword arguments of ops.step_init / ops.step_advance, under their names
        self.hyper = dict(base_lr=float(base_lr), max_iterations=float(max_iterations), ema_decay=float(ema_decay),
                          consistency=float(consistency), rampup=float(consistency_rampup), ramp_div=150,
                          cons_start_iter=int(cons_start_iter), lr_post_increment=bool(lr_post_increment))
        self.momentum, self.weight_decay = momentum, weight_decay
        self.pg = process_group
        self.world = dist.world_size(process_group)
        self.use_tape = STEP_TAPE if use_tape is None else bool(use_tape)
        self.state = ops.new_step_state()
        ops.step_init(self.state, seed, iter_num, **self.hyper)
        for net, stream in zip(self._nets, rng_streams):
            net.step_state, net.rng_stream = self.state, stream
        names = ((("momentum_buf", "out"),) if len(students) == 1 else
                 tuple((f"mom{i}", f"out{i}") for i in range(1, len(students) + 1)))
        for net, (mom, out) in zip(students, names):
            setattr(self, mom, torch.zeros_like(net.flat_param))
            setattr(self, out, torch.zeros(16, dtype=torch.float32, device="cuda"))
        self.iter_num = iter_num

    # ---- one iteration ----
    def _step(self, volume, label, *inject):
        """The body of every ``step()``.  ``inject``: the values a parity test passes in place of the step's device-side draws
        (noise, mix factors, rotation); one that is not None keeps the step eager.  Returns the device scalar buffer(s)."""
        if not all(net.training for net in self._nets):
            raise RuntimeError(self.TRAIN_MODE)
        if all(x is None for x in inject):
            self._replay(volume, label, *inject)
        else:
            self._run(volume, label, *inject)
        self.iter_num += 1
        if len(self._students) == 1:
            return self.out
        return tuple(getattr(self, f"out{i}") for i in range(1, len(self._students) + 1))

    def _replay(self, volume, label, *none):
        """A step on its own device-side draws: through the launch tape unless the trainer is eager."""
        if self.use_tape:
            self._tape_step(lambda v, l: self._run(v, l, *none), (volume, label))
        else:
            self._run(volume, label, *none)

    # ---- the pieces of _run ----
    def _scratch(self, name, like, shape=None):
        """The input buffer ``self.<name>`` of ``like``'s shape (or ``shape``), dtype and device: allocated on first use and
        again when the batch geometry changes."""
        shape = tuple(like.shape if shape is None else shape)
        buf = getattr(self, name)
        if buf is None or tuple(buf.shape) != shape:
            buf = torch.empty(shape, dtype=like.dtype, device=like.device)
            setattr(self, name, buf)
        return buf

    def _noised(self, unl, noise):
        """The teacher's input: the unlabeled half plus clipped Gaussian noise drawn on the device (``noise``: injected, parity
        tests only)."""
        ema_in = self._scratch("_ema_in", unl)
        if noise is None:
            ops.teacher_noise(unl, ema_in, self.state)
        else:
            torch.add(unl, noise, out=ema_in)
        return ema_in

    def _beside(self, side_fn, main_fn):
        """Two independent pieces of work; returns ``(side_fn(), main_fn())``.  With TWO_STREAM ``side_fn`` is enqueued first, on
        the side stream, between a fork (side waits for main) and a join (main waits for side), and fills the CUs that
        ``main_fn``'s launch tails and small deep layers leave idle.  Without, ``main_fn`` then ``side_fn`` on the one stream.
        Same kernels, same order per network, same reduction trees: bit-identical training either way."""
        if not TWO_STREAM:
            res = main_fn()
            return side_fn(), res
        main = torch.cuda.current_stream()
        if self._side is None:
            self._side = torch.cuda.Stream()
        _lib.wait_stream(self._side, main)
        with torch.cuda.stream(self._side):
            side_res = side_fn()
        res = main_fn()
        _lib.wait_stream(main, self._side)
        return side_res, res

    def _backward_pair(self, side):
        """The backward of both students, student ``side`` (0 / 1) beside the other one, with both exchanges in flight until
        one wait at the end; returns the two 1/world scales.  With bucketers both are begun first (a host-side reset); the
        collectives are ENQUEUED by this thread in program order -- the side student's buckets, then the other one's -- the same
        on every rank.  The side student's bucketer is built with ``defer_tail``: its tail bucket goes out in ``finish``, so the
        in-order RCCL stream does not hold the other student's early buckets behind the end of the side backward."""
        nets, (b1, b2) = self._students, self._bucketers
        main = 1 - side
        if b1 is None:
            self._beside(nets[side].backward_raw, nets[main].backward_raw)
            return [_lib.tape_call(dist.sync_gradients, net.flat_grad, self.pg) for net in nets]
        bs = (b1, b2)
        _lib.tape_call(b1.begin)
        _lib.tape_call(b2.begin)

        def main_backward():
            nets[main].backward_raw(on_progress=bs[main].advance)
            if not TWO_STREAM:
                # one stream: this backward ran first and is complete; what is left of its buckets goes out now, before the
                # other student's backward, and travels beside it
                _lib.tape_call(bs[main].advance, 0, True)

        self._beside(lambda: nets[side].backward_raw(on_progress=bs[side].advance), main_backward)
        return [_lib.tape_call(b1.finish), _lib.tape_call(b2.finish)]

    def _backward_beside(self, side, main):
        """The backwards of the students ``side`` (indices into the students), one after another on the side stream, beside
        those of the students ``main`` on the main stream.  No exchange is begun here: the caller follows with blocking ones."""
        nets = self._students
        self._beside(lambda: [nets[i].backward_raw() for i in side], lambda: [nets[i].backward_raw() for i in main])

    def _finish_step(self, *updates):
        """Fused SGD (+ EMA of the teacher) for every ``(student, momentum buffer, teacher parameters or None, grad scale)``, then
        the schedule: iteration, learning rate, EMA alpha and consistency weight advance on the device."""
        for net, mom, ema_param, grad_scale in updates:
            ops.sgd_ema_step(net.flat_param, net.flat_grad, mom, ema_param, momentum=self.momentum,
                             weight_decay=self.weight_decay, grad_scale=grad_scale, state=self.state)
        self._advance_schedule()

    def _advance_schedule(self):
        """The device-side schedule after the optimizer: the Mean-Teacher family's rule (a trainer whose script has another
        one overrides this)."""
        ops.step_advance(self.state, **self.hyper)

    def _pair_losses(self):
        """Host copies of ``out1`` / ``out2`` and what every two-student step reports from them."""
        a, b = self.out1.cpu(), self.out2.cpu()
        return a, b, dict(loss=a[0].item() + b[0].item(), model1_loss=a[0].item(), model2_loss=b[0].item(),
                          loss1_ce=a[1].item(), loss1_dice=a[2].item(), pseudo_supervision1=a[3].item(),
                          loss2_ce=b[1].item(), loss2_dice=b[2].item(), pseudo_supervision2=b[3].item(),
                          consistency_weight=a[4].item())


class _TeacherStudentStep(_Step):
    """One student and its EMA teacher: what the Mean-Teacher step, UA-MT and ICT have in common.  Dropout streams: student 1,
    teacher 2."""

    def __init__(self, model, ema_model, *, labeled_bs, num_classes, base_lr=0.01, max_iterations=30000,
                 ema_decay=0.99, consistency=0.1, consistency_rampup=200.0, cons_start_iter=0, seed=1337,
                 iter_num=0, momentum=0.9, weight_decay=1e-4, process_group=None, use_tape=None):
        if model.flat_param.numel() != ema_model.flat_param.numel():
            raise RuntimeError("student and teacher must be the same architecture")
        self.model, self.ema_model = model, ema_model
        self._setup((model,), (ema_model,), (1, 2), labeled_bs=labeled_bs, num_classes=num_classes, base_lr=base_lr,
                    max_iterations=max_iterations, ema_decay=ema_decay, consistency=consistency,
                    consistency_rampup=consistency_rampup, cons_start_iter=cons_start_iter, seed=seed, iter_num=iter_num,
                    momentum=momentum, weight_decay=weight_decay, process_group=process_group, use_tape=use_tape)
        self._bucketer = make_bucketer(model, process_group)

    def _backward_and_finish(self):
        grad_scale = backward_and_sync(self.model, self.pg, self._bucketer)   # the step's only exchange
        self._finish_step((self.model, self.momentum_buf, self.ema_model.flat_param, grad_scale))

    def losses(self):
        """Host copy of the last step's scalars (one small D2H)."""
        o = self.out.cpu()
        return dict(loss=o[0].item(), loss_ce=o[1].item(), loss_dice=o[2].item(),
                    consistency_loss=o[3].item(), consistency_weight=o[4].item())


class MeanTeacherTrainer(_TeacherStudentStep):
    """Mean Teacher (reference code/train_mean_teacher_2D.py:202-236, code/train_mean_teacher_3D.py:134-166): student forward
    on the batch, EMA-teacher forward on the noised unlabeled half, softmax / CE / Dice / softmax-MSE consistency in one fused
    loss tail.  ``use_graph=True`` (single GPU) captures the step once into a hipGraph and replays that instead of the tape."""

    TRAIN_MODE = "Mean-Teacher step runs both networks in train mode (reference never calls .eval())"

    def __init__(self, model, ema_model, *, use_graph=False, **kw):
        super().__init__(model, ema_model, **kw)
        # a captured replay of a step that contains an RCCL collective is not verified on hardware: single-GPU only
        self.use_graph = bool(use_graph) and self.world == 1
        self.use_tape = self.use_tape and not self.use_graph
        self._graph = None
        self._static = None

    # ---- the step (eager form; also what gets recorded or captured) ----
    def _run(self, volume, label, noise):
        L = self.labeled_bs
        ema_in = self._noised(volume[L:].contiguous(), noise)
        # the two forwards are independent: the teacher's is half the batch and has no backward
        t_logits, s_logits = self._beside(lambda: self.ema_model.forward_raw(ema_in, no_backward=True),
                                          lambda: self.model.forward_raw(volume))
        ops.loss_tail(s_logits, t_logits, label[:L].contiguous(), L, self.out,
                      dlogits=self.model.logits_grad_buffer(), state=self.state)
        self._backward_and_finish()

    def step(self, volume_batch, label_batch, noise=None):
        """One iteration on device tensors; returns the device scalar buffer
        ``[loss, loss_ce, loss_dice, consistency_loss, consistency_weight, ...]`` (no host sync)."""
        return self._step(volume_batch, label_batch, noise)

    def _replay(self, volume, label, noise):
        if self.use_graph:
            self._step_graph(volume, label)
        else:
            super()._replay(volume, label, noise)

    # ---- hipGraph capture / replay ----
    def _step_graph(self, volume, label):
        if self._graph is None:
            self._static = (volume.clone(), label.clone())
            # one eager warm-up builds plans and scratch buffers outside the capture
            # (it is a real training step on the real batch)
            self._run(self._static[0], self._static[1], None)
            torch.cuda.synchronize()
            self._graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(self._graph):
                self._run(self._static[0], self._static[1], None)
            # capture does not execute: the warm-up above WAS this call's step
            return
        self._static[0].copy_(volume)
        self._static[1].copy_(label)
        self._graph.replay()


class UAMTTrainer(_TeacherStudentStep):
    """Uncertainty-aware Mean Teacher (reference code/train_uncertainty_aware_mean_teacher_3D.py:134-189,
    code/train_uncertainty_aware_mean_teacher_2D.py:146-201): the Mean-Teacher step plus T = 8 MC-dropout
    teacher predictions (4 forwards on ``repeat(unlabeled, 2)`` with fresh noise), whose mean-probability
    entropy masks the consistency term.  Every teacher forward runs in train mode (dropout active, BatchNorm
    running statistics updated 5 times per step, as in the reference)."""

    T = 8
    TRAIN_MODE = "UA-MT runs both networks in train mode (MC dropout needs the teacher's dropout)"
    _rep_in = None
    _mean_probs = None

    def __init__(self, model, ema_model, *, use_tape=None, **kw):
        # eager only, whatever the caller asks for: the MC passes cycle the teacher through RNG sub-streams set from
        # Python, which a recorded step would not repeat
        super().__init__(model, ema_model, use_tape=False, **kw)

    def _run(self, volume, label, noise, mc_noise):
        L = self.labeled_bs
        unl = volume[L:].contiguous()
        U = unl.shape[0]
        ema_in = self._noised(unl, noise)
        rep_in = self._scratch("_rep_in", unl, (2 * U,) + tuple(unl.shape[1:]))

        def teacher_passes():
            self.ema_model.rng_stream = 2
            t_logits = self.ema_model.forward_raw(ema_in, no_backward=True)
            if self._mean_probs is None or self._mean_probs.shape != t_logits.shape:
                self._mean_probs = torch.empty_like(t_logits)
            for i in range(self.T // 2):
                for r in range(2):
                    half = rep_in[r * U:(r + 1) * U]
                    if mc_noise is None:
                        ops.teacher_noise(unl, half, self.state, salt=0x7EAC4E5 + 1 + 2 * i + r)
                    else:
                        torch.add(unl, mc_noise[i][r * U:(r + 1) * U], out=half)
                self.ema_model.rng_stream = 3 + i          # a fresh dropout stream per MC pass
                mc_logits = self.ema_model.forward_raw(rep_in, no_backward=True)
                ops.softmax_mean_accumulate(mc_logits, self._mean_probs, 2, 1.0 / self.T, first=(i == 0))
            self.ema_model.rng_stream = 2
            return t_logits

        # the five teacher forwards (one plain, four MC passes: sequential, they share the teacher's buffers) only meet the
        # student in the loss tail
        t_logits, s_logits = self._beside(teacher_passes, lambda: self.model.forward_raw(volume))
        ops.uamt_tail(s_logits, t_logits, self._mean_probs, label[:L].contiguous(), L, self.out,
                      self.hyper["max_iterations"], dlogits=self.model.logits_grad_buffer(), state=self.state)
        self._backward_and_finish()

    def step(self, volume_batch, label_batch, noise=None, mc_noise=None):
        return self._step(volume_batch, label_batch, noise, mc_noise)

    def losses(self):
        d = super().losses()
        o = self.out.cpu()
        C = self.num_classes
        d.update(unmasked_voxels=o[5 + C].item(), threshold=o[6 + C].item())
        return d


def ict_split(batch_size, labeled_bs):
    """M = labeled_bs // 2, the number of mixed samples of an ICT step.  The reference splits the unlabeled part
    volume[L:] at M into x0 and x1 and broadcasts [M]-shaped factors over both, which only works when the batch holds
    exactly L + 2M samples (train_interpolation_consistency_training_2D.py:156-165): anything else is a ValueError."""
    B, L = int(batch_size), int(labeled_bs)
    if L < 2:
        raise ValueError(f"ICT needs labeled_bs >= 2 (labeled_bs // 2 mixed samples); got labeled_bs={L}")
    M = L // 2
    if B - L != 2 * M:
        raise ValueError(f"ICT needs batch_size - labeled_bs == 2 * (labeled_bs // 2) = {2 * M} unlabeled samples; "
                         f"got batch_size={B}, labeled_bs={L}")
    return M


class ICTTrainer(_TeacherStudentStep):
    """Interpolation Consistency Training (reference code/train_interpolation_consistency_training_2D.py:150-190,
    _3D.py:140-182, _2D_ViT.py:190-235).  With L = labeled_bs and M = L // 2 the unlabeled samples x0 = volume[L:L+M]
    and x1 = volume[L+M:] are mixed with per-sample factors lam ~ Beta(ict_alpha, ict_alpha) drawn on the device; the
    student sees cat([volume[:L], x0 * (1 - lam) + x1 * lam]) (L + M samples) and is pulled towards
    softmax(T(x0)) * (1 - lam) + softmax(T(x1)) * lam.  The teacher runs two train-mode forwards (BatchNorm running
    statistics updated twice per step), with no input noise.  SGD, poly LR, EMA and the consistency ramp are those of
    the Mean-Teacher step; there is no ``iter_num < 1000`` gate."""

    TEACHER_STREAMS = (2, 3)        # Philox dropout sub-streams of the two teacher passes (the student's is 1)
    TRAIN_MODE = "ICT runs both networks in train mode (the reference never calls ema_model.eval())"
    _mix_in = None

    def __init__(self, model, ema_model, *, ict_alpha=0.2, **kw):
        if not float(ict_alpha) > 0.0:
            raise ValueError(f"ict_alpha must be > 0, got {ict_alpha}")
        super().__init__(model, ema_model, **kw)
        self.ict_alpha = float(ict_alpha)
        self.mix_factors = None     # [M] device tensor: the factors of the last step

    def _run(self, volume, label, mix_factors):
        L = self.labeled_bs
        M = ict_split(volume.shape[0], L)
        if self.mix_factors is None or self.mix_factors.numel() != M:
            self.mix_factors = torch.empty(M, dtype=torch.float32, device=volume.device)
        if mix_factors is None:
            ops.beta_sample(self.mix_factors, self.ict_alpha, self.state)
        else:
            self.mix_factors.copy_(mix_factors.reshape(-1))        # injected factors: parity tests only
        mix_in = self._scratch("_mix_in", volume, (L + M,) + tuple(volume.shape[1:]))
        ops.ict_mix(volume, self.mix_factors, L, mix_in)
        x0, x1 = volume[L:L + M], volume[L + M:]
        ema = self.ema_model

        def teacher_passes():
            # two forwards of one shape: the second uses a second plan so that the first one's logits survive it
            ema.rng_stream = self.TEACHER_STREAMS[0]
            t0 = ema.forward_raw(x0, no_backward=True)
            ema.rng_stream = self.TEACHER_STREAMS[1]
            t1 = ema.forward_raw(x1, no_backward=True, slot=1)
            ema.rng_stream = self.TEACHER_STREAMS[0]
            return t0, t1

        # the teacher passes read only the raw batch
        (t0, t1), s_logits = self._beside(teacher_passes, lambda: self.model.forward_raw(mix_in))
        ops.ict_tail(s_logits, t0, t1, self.mix_factors, label[:L].contiguous(), L, self.out,
                     dlogits=self.model.logits_grad_buffer(), state=self.state)
        self._backward_and_finish()

    def step(self, volume_batch, label_batch, mix_factors=None):
        """One ICT iteration on device tensors; ``mix_factors`` ([M] or [M,1,1,1(,1)]) replaces the device Beta draw
        (parity tests).  Returns the device scalar buffer of MeanTeacherTrainer.step (no host sync)."""
        M = ict_split(volume_batch.shape[0], self.labeled_bs)
        if mix_factors is not None and mix_factors.numel() != M:
            raise ValueError(f"mix_factors must hold labeled_bs // 2 = {M} values, got {mix_factors.numel()}")
        return self._step(volume_batch, label_batch, mix_factors)


def fixmatch_split(batch_size, labeled_bs):
    """U = batch_size - labeled_bs, the unlabeled samples of a FixMatch step.  ValueError unless 1 <= labeled_bs <
    batch_size: the supervised CE / Dice need a labeled sample and the pseudo-label terms an unlabeled one (the reference's
    CrossEntropyLoss of an empty slice is NaN)."""
    B, L = int(batch_size), int(labeled_bs)
    if not 1 <= L < B:
        raise ValueError(f"FixMatch needs 1 <= labeled_bs < batch_size; got batch_size={B}, labeled_bs={L}")
    return B - L


class FixMatchTrainer(_TeacherStudentStep):
    """FixMatch with complementary learning (reference code/train_Fixmatch_CNN_2D.py:247-301): ONE network, two train-mode
    forwards per step -- on the weak batch, then on its colour-jittered (strong) copy, so BatchNorm running statistics are
    updated twice, in that order -- and the loss of ``mis_fixmatch_tail``: CE + Dice on the labeled weak rows, and, times
    w = consistency * sigmoid_rampup(iter // 150) (no ``iter_num < 1000`` gate), CE + Dice of the strong unlabeled rows
    against confidence-masked pseudo labels of the weak pass plus the complementary cross-entropy scaled by the squared
    adaptive weight, which is differentiated through.  SGD (momentum 0.9, wd 1e-4), poly LR and the EMA of the student into
    ``ema_model`` in the Mean-Teacher order; the reference updates ``ema_model`` and never runs it, so neither does this step.

    The strong batch is made inside the step (``mis_color_jitter``) from factors drawn on the device under (seed, iter_num),
    so a replayed launch tape jitters every iteration anew; ``jitter_factors`` ([B, 3]: beta, gamma, order) holds the last
    step's.  The two passes run on two plans (strong on ``slot=1``); the strong backward's flat gradient is stashed and
    added to the weak one's (``mis_grad_combine``).  With a process group the sum is exchanged once, after the second
    backward, by a blocking all-reduce."""

    PASS_STREAMS = (1, 2)           # Philox dropout sub-streams of the weak and the strong pass
    TRAIN_MODE = "FixMatch runs both passes in train mode (the reference never calls .eval() inside the loop)"
    _strong_in = None

    def __init__(self, model, ema_model, *, conf_thresh=0.8, **kw):
        super().__init__(model, ema_model, **kw)
        self._bucketer = None                     # two backwards fill the flat gradient: one exchange after the second
        self.conf_thresh = float(conf_thresh)
        self.jitter_factors = None                # [B, 3] device tensor: (beta, gamma, order) of the last step
        self._stash = torch.zeros_like(model.flat_grad)

    def _run(self, volume, label, strong, jitter):
        L, m = self.labeled_bs, self.model
        B = volume.shape[0]
        if strong is None:
            strong = self._scratch("_strong_in", volume)
            if self.jitter_factors is None or self.jitter_factors.shape[0] != B:
                self.jitter_factors = torch.zeros((B, 3), dtype=torch.float32, device=volume.device)
            params = None if jitter is None else jitter.to(device=volume.device, dtype=torch.float32).reshape(B, 3).contiguous()
            ops.color_jitter(volume, strong, params=params, state=self.state, drawn=self.jitter_factors)
        m.rng_stream = self.PASS_STREAMS[0]
        zw = m.forward_raw(volume)
        pw = m.last_pass()
        m.rng_stream = self.PASS_STREAMS[1]
        zs = m.forward_raw(strong, slot=1)         # a plan of its own: the weak pass's activations and logits survive it
        ps = m.last_pass()
        m.rng_stream = self.PASS_STREAMS[0]
        ops.fixmatch_tail(zw, zs, label[:L].contiguous(), L, self.out, d_weak=m.logits_grad_buffer(pw),
                          d_strong=m.logits_grad_buffer(ps), conf_thresh=self.conf_thresh, state=self.state)
        # each backward writes (does not add to) the flat gradient buffer: see DeepCoTrainingTrainer._run for the ordering
        m.backward_raw(pass_=ps)
        ops.grad_combine(self._stash, m.flat_grad, accumulate=False)
        m.backward_raw(pass_=pw)
        ops.grad_combine(m.flat_grad, self._stash, accumulate=True)
        grad_scale = _lib.tape_call(dist.sync_gradients, m.flat_grad, self.pg)     # the step's only exchange
        self._finish_step((m, self.momentum_buf, self.ema_model.flat_param, grad_scale))

    def step(self, weak_batch, label_batch, strong=None, jitter=None):
        """One iteration on device tensors [B, 1, H, W] / [B, H, W].  ``strong`` ([B, 1, H, W]) replaces the strong batch,
        ``jitter`` ([B, 3]: beta, gamma, order) the drawn factors; either keeps the step eager (parity tests, or a loader
        that augments per item).  Returns the device scalar buffer, ``ops.FIXMATCH_OUT`` by position (no host sync)."""
        if weak_batch.dim() != 4 or weak_batch.shape[1] != 1:
            raise ValueError(f"FixMatch runs the 2-D networks on [B, 1, H, W]; got {tuple(weak_batch.shape)}")
        B = weak_batch.shape[0]
        fixmatch_split(B, self.labeled_bs)
        if strong is not None and (jitter is not None or tuple(strong.shape) != tuple(weak_batch.shape)):
            raise ValueError("strong must have the weak batch's shape and excludes jitter")
        if jitter is not None and jitter.numel() != 3 * B:
            raise ValueError(f"jitter must hold (beta, gamma, order) per sample: {3 * B} values, got {jitter.numel()}")
        return self._step(weak_batch, label_batch, strong, jitter)

    def losses(self):
        o = self.out.cpu()
        return {k: o[i].item() for i, k in enumerate(ops.FIXMATCH_OUT)}


def rotation_schedule(seed, n):
    """The rotation counts of the reference's deep co-training: ``random.seed(seed)`` in the main process, then one
    ``random.randrange(0, 4)`` per iteration (code/train_deep_co_training_2D.py:141, :248).  Nothing else of that process
    draws from ``random`` (the augmentation's draws run in the DataLoader workers), so entry i is iteration i's k."""
    r = random.Random(seed)
    return [r.randrange(0, 4) for _ in range(int(n))]


def dct_split(batch_size, labeled_bs, patch_size=None):
    """U = batch_size - labeled_bs, the unlabeled samples of a deep co-training step.  ValueError unless
    1 <= labeled_bs < batch_size (CE / Dice need a labeled sample, the consistency mean an unlabeled one) and, when given,
    the patch is square: an odd k turns H x W into W x H, and the step runs on static plans of one shape."""
    B, L = int(batch_size), int(labeled_bs)
    if not 1 <= L < B:
        raise ValueError(f"deep co-training needs 1 <= labeled_bs < batch_size; got batch_size={B}, labeled_bs={L}")
    if patch_size is not None and (len(patch_size) != 2 or int(patch_size[0]) != int(patch_size[1])):
        raise ValueError(f"deep co-training rotates by 90 degrees: the patch must be square, got {list(patch_size)}")
    return B - L


class DeepCoTrainingTrainer(_Step):
    """Deep co-training, rotation consistency (reference code/train_deep_co_training_2D.py:134-167,
    _2D_ViT.py:172-205): ONE network, two train-mode forwards per step -- pass A on the batch, pass R on
    ``rot90(volume[L:], k)`` -- and ``0.5 * (CE + Dice)(A[:L]) + w * 0.5 * (mean((Q.detach() - rot P)^2) +
    mean((Q - (rot P).detach())^2))`` with P = softmax(A[L:]), Q = softmax(R), w = consistency * sigmoid_rampup(iter // 150)
    (no ``iter_num < 1000`` gate).  Plain SGD (momentum 0.9, wd 1e-4), poly LR in the Mean-Teacher order; no EMA, no teacher.

    k comes from ``rotation_schedule(seed, max_iterations)`` held on the device and read there at ``state.iter_num``, so a
    replayed launch tape rotates by each iteration's own k.  The network is differentiated through both passes: they run
    on two plans (R on ``slot=1``), each backward writes the flat gradient buffer, so R's gradient is stashed and added to
    A's (``mis_grad_combine``) before the optimizer.  With a process group the summed buffer is exchanged ONCE, after the
    second backward, by a blocking all-reduce: this trainer does not overlap the exchange with the backward."""

    PASS_STREAMS = (1, 2)           # Philox dropout sub-streams of pass A and pass R
    TRAIN_MODE = "deep co-training runs both passes in train mode (the reference never calls .eval() there)"
    _rot_in = None

    def __init__(self, model, *, labeled_bs, num_classes, base_lr=0.01, max_iterations=30000, consistency=0.1,
                 consistency_rampup=200.0, seed=1337, iter_num=0, momentum=0.9, weight_decay=1e-4, process_group=None,
                 use_tape=None, patch_size=None):
        if patch_size is not None:
            dct_split(labeled_bs + 1, labeled_bs, patch_size)
        self.model = model
        self._setup((model,), (), self.PASS_STREAMS[:1], labeled_bs=int(labeled_bs), num_classes=num_classes,
                    base_lr=base_lr, max_iterations=max_iterations, consistency=consistency,
                    consistency_rampup=consistency_rampup, seed=seed, iter_num=iter_num, momentum=momentum,
                    weight_decay=weight_decay, process_group=process_group, use_tape=use_tape)
        self.schedule = torch.tensor(rotation_schedule(seed, max(int(max_iterations), 1)), dtype=torch.int32,
                                     device="cuda")
        self._stash = torch.zeros_like(model.flat_grad)

    def _run(self, volume, label, rot_k):
        L, m = self.labeled_bs, self.model
        rot_in = self._scratch("_rot_in", volume[L:])       # square planes: one shape for every k
        k = -1 if rot_k is None else int(rot_k)
        ops.rot90(volume[L:], rot_in, k=k, sched=self.schedule, state=self.state)
        # A then R, one after the other on this stream: BatchNorm running statistics are updated twice, in the reference's
        # order.  R runs on a plan of its own (slot 1), so A's activations and logits survive it.
        m.rng_stream = self.PASS_STREAMS[0]
        a = m.forward_raw(volume)
        pa = m.last_pass()
        m.rng_stream = self.PASS_STREAMS[1]
        r = m.forward_raw(rot_in, slot=1)
        pr = m.last_pass()
        m.rng_stream = self.PASS_STREAMS[0]
        ops.dct_tail(a, r, label[:L].contiguous(), L, self.out, dA=m.logits_grad_buffer(pa), dR=m.logits_grad_buffer(pr),
                     k=k, sched=self.schedule, state=self.state)
        # A backward writes (does not add to) the flat gradient buffer.  The stash copy is enqueued on this stream after R's
        # backward has joined its weight-gradient side stream, and every side-stream section of A's backward starts with a
        # wait for this stream (Plan.backward / ConvOp.bwd / LinearOp.bwd): no weight gradient of A lands before the copy.
        m.backward_raw(pass_=pr)
        ops.grad_combine(self._stash, m.flat_grad, accumulate=False)
        m.backward_raw(pass_=pa)
        ops.grad_combine(m.flat_grad, self._stash, accumulate=True)
        grad_scale = _lib.tape_call(dist.sync_gradients, m.flat_grad, self.pg)     # the step's only exchange
        self._finish_step((m, self.momentum_buf, None, grad_scale))

    def step(self, volume_batch, label_batch, rot_k=None):
        """One iteration on device tensors [B, 1, H, W] / [B, H, W]; ``rot_k`` (0..3) replaces the scheduled rotation
        (parity tests, eager).  Returns the device scalar buffer ``[loss, loss_ce, loss_dice, consistency_loss,
        consistency_weight, k, ...]`` (no host sync)."""
        if volume_batch.dim() != 4:
            raise ValueError(f"deep co-training runs the 2-D networks on [B, C, H, W]; got {tuple(volume_batch.shape)}")
        dct_split(volume_batch.shape[0], self.labeled_bs, tuple(volume_batch.shape[2:]))
        if rot_k is not None and rot_k not in (0, 1, 2, 3):
            raise ValueError(f"rot_k must be 0, 1, 2 or 3, got {rot_k}")
        return self._step(volume_batch, label_batch, rot_k)

    def losses(self):
        o = self.out.cpu()
        return dict(loss=o[0].item(), loss_ce=o[1].item(), loss_dice=o[2].item(), consistency_loss=o[3].item(),
                    consistency_weight=o[4].item(), rot_k=int(o[5].item()))


class CrossTeachingTrainer(_Step):
    """Cross teaching between a CNN and a Transformer (reference
    code/train_cross_teaching_between_cnn_transformer_2D.py:216-263): two students see the whole batch, each is
    supervised on the labeled half and by the OTHER network's arg-max pseudo labels (Dice) on the unlabeled
    half; ``loss = model1_loss + model2_loss``, two SGD steps, no EMA, no noise.  The learning rate follows the
    post-increment rule of that script (:257-263)."""

    TRAIN_MODE = "cross teaching trains both networks (train mode)"

    def __init__(self, model1, model2, *, labeled_bs, num_classes, base_lr=0.01, max_iterations=30000,
                 consistency=0.1, consistency_rampup=200.0, seed=1337, iter_num=0, momentum=0.9, weight_decay=1e-4,
                 process_group=None, pseudo_ce=False, use_tape=None):
        # pseudo_ce=True: cross pseudo supervision (code/train_cross_pseudo_supervision_{2D,3D}.py): the same step
        # with a cross-entropy pseudo-supervision term instead of Dice
        self.pseudo_ce = bool(pseudo_ce)
        self.model1, self.model2 = model1, model2
        self._setup((model1, model2), (), (1, 2), labeled_bs=labeled_bs, num_classes=num_classes, base_lr=base_lr,
                    max_iterations=max_iterations, consistency=consistency, consistency_rampup=consistency_rampup,
                    lr_post_increment=True, seed=seed, iter_num=iter_num, momentum=momentum, weight_decay=weight_decay,
                    process_group=process_group, use_tape=use_tape)
        # model2 is the side-stream student (_backward_pair): its tail bucket is deferred
        self._bucketers = (make_bucketer(model1, process_group),
                           make_bucketer(model2, process_group, defer_tail=TWO_STREAM))

    def step(self, volume_batch, label_batch):
        return self._step(volume_batch, label_batch)

    def _run(self, volume_batch, label_batch):
        L = self.labeled_bs
        lab = label_batch[:L].contiguous()
        # the two students only meet in the loss tails: model2's forward and backward run beside model1's
        o2, o1 = self._beside(lambda: self.model2.forward_raw(volume_batch), lambda: self.model1.forward_raw(volume_batch))
        ops.cross_teaching_tail(o1, o2, lab, L, self.out1, dlogits=self.model1.logits_grad_buffer(), state=self.state,
                                pseudo_ce=self.pseudo_ce)
        ops.cross_teaching_tail(o2, o1, lab, L, self.out2, dlogits=self.model2.logits_grad_buffer(), state=self.state,
                                pseudo_ce=self.pseudo_ce)
        scales = self._backward_pair(side=1)
        self._finish_step((self.model1, self.mom1, None, scales[0]), (self.model2, self.mom2, None, scales[1]))

    def losses(self):
        return self._pair_losses()[2]


def contrastive_split(batch_size, labeled_bs):
    """U = batch_size - labeled_bs, the unlabeled samples of a contrastive cross-teaching step.  ValueError unless
    labeled_bs is even and 2 <= labeled_bs < batch_size: the supervised contrastive term pairs the labeled rows 0::2 of one
    student with the rows 1::2 of the other (the reference asserts equal feature shapes), and ConLoss needs an unlabeled row."""
    B, L = int(batch_size), int(labeled_bs)
    if L < 2 or L % 2 or not L < B:
        raise ValueError(f"contrastive cross teaching needs an even labeled_bs with 2 <= labeled_bs < batch_size; got "
                         f"batch_size={B}, labeled_bs={L}")
    return B - L


class ContrastiveCrossTrainer(_Step):
    """Contrastive cross teaching (reference code/train_Contrastive_Cross_CNN_2D.py:212-283; _CNN_ViT_2D.py is the same
    step with the SwinUnet as ``model2``): cross teaching through Dice on each other's arg-max pseudo labels, plus two
    pixel-wise contrastive terms between the students' logits seen through small frozen heads --

        Lc_l = contrastive_loss_sup(classifier_1(z1[:L][0::2]), classifier_2(z2[:L][1::2]))
        Lc_u = ConLoss(projector_1(z1[L:]), projector_2(z2[L:]))
        loss = 2 * (sup_1 + sup_2) + 0.5 * (Lc_l + Lc_u) + 1.25 * w * (ps_1 + ps_2)

    Both losses detach the key side, so only ``model1`` receives a contrastive gradient: on the labeled rows 0, 2, ...
    through ``classifier_1`` and on every unlabeled row through ``projector_1``.  The four heads are in no optimizer
    (``HipNet.frozen``): they keep their initial weights, run in train mode (BatchNorm batch statistics of the sub-batch,
    running buffers updated) and their backward forms the input gradient only.  ``ops.contrastive_cross_tail`` adds those
    input gradients into ``model1``'s logits gradient in the pass that writes it.  ``SCALES`` is the one place the
    script's 2 / 0.5 / 1.25 stand.

    w = consistency * ramp_up_function(iter_num // iters_per_epoch, rampup) and the script's own learning-rate rule
    (:274-278, 1e-4 based once past half of max_iterations) advance on the device (``mis_contrastive_step_advance``), so the
    taped step stays right across an epoch boundary and the LR switch.  With a process group the heads are broadcast from
    rank 0 once, here, and nothing of theirs is exchanged afterwards; BatchNorm statistics stay per rank."""

    TRAIN_MODE = "contrastive cross teaching runs both students and the four heads in train mode"
    SCALES = dict(sup=2.0, contrastive=0.5, pseudo=1.25)          # reference :261

    def __init__(self, model1, model2, classifier_1, classifier_2, projector_1, projector_2, *, labeled_bs, num_classes,
                 iters_per_epoch, base_lr=0.01, max_iterations=30000, consistency=0.1, consistency_rampup=200.0,
                 seed=1337, iter_num=0, momentum=0.9, weight_decay=1e-4, temperature=0.07, process_group=None,
                 use_tape=None):
        contrastive_split(int(labeled_bs) + 1, labeled_bs)        # an odd labeled_bs is refused before any launch
        if int(iters_per_epoch) < 1:
            raise ValueError(f"iters_per_epoch must be >= 1, got {iters_per_epoch}")
        heads = (classifier_1, classifier_2, projector_1, projector_2)
        if not all(getattr(h, "frozen", False) for h in heads):
            raise RuntimeError("the contrastive heads are in no optimizer: pass HipNets with frozen = True "
                               "(networks.projector)")
        self.model1, self.model2 = model1, model2
        self.classifier_1, self.classifier_2, self.projector_1, self.projector_2 = heads
        self._setup((model1, model2), heads, (1, 2, 3, 4, 5, 6), labeled_bs=int(labeled_bs), num_classes=num_classes,
                    base_lr=base_lr, max_iterations=max_iterations, consistency=consistency,
                    consistency_rampup=consistency_rampup, lr_post_increment=True, seed=seed, iter_num=iter_num,
                    momentum=momentum, weight_decay=weight_decay, process_group=process_group, use_tape=use_tape)
        # this script's schedule instead of the Mean-Teacher family's (_setup wrote that one into the state)
        self.sched = dict(base_lr=float(base_lr), max_iterations=float(max_iterations), consistency=float(consistency),
                          rampup=float(consistency_rampup), iters_per_epoch=int(iters_per_epoch))
        ops.contrastive_step_init(self.state, seed, iter_num, **self.sched)
        self.temperature = float(temperature)
        self.out_cl = torch.zeros(4, dtype=torch.float32, device="cuda")      # ops.patch_nce scalars: Lc_l, ...
        self.out_cu = torch.zeros(4, dtype=torch.float32, device="cuda")      # ... and Lc_u
        for h in heads:
            dist.broadcast_state([h.flat_param] + list(h.buffers()), group=process_group)
            h.weights_changed()
        # model2 is the side-stream student (_backward_pair): its tail bucket is deferred
        self._bucketers = (make_bucketer(model1, process_group),
                           make_bucketer(model2, process_group, defer_tail=TWO_STREAM))

    def _advance_schedule(self):
        ops.contrastive_step_advance(self.state, **self.sched)

    def step(self, volume_batch, label_batch):
        """One iteration on device tensors [B, 1, H, W] / [B, H, W]; returns the two device scalar buffers
        (``ops.CONTRASTIVE_OUT`` by position; no host sync)."""
        contrastive_split(volume_batch.shape[0], self.labeled_bs)
        return self._step(volume_batch, label_batch)

    def _run(self, volume_batch, label_batch):
        L, s = self.labeled_bs, self.SCALES
        lab = label_batch[:L].contiguous()
        o2, o1 = self._beside(lambda: self.model2.forward_raw(volume_batch), lambda: self.model1.forward_raw(volume_batch))
        cls1, cls2, prj1, prj2 = self.classifier_1, self.classifier_2, self.projector_1, self.projector_2
        # the key side is detached by both losses: forward only, beside the query side (batch-strided views, not copies)
        z1, z2 = o1.squeeze(2), o2.squeeze(2)       # [B, C, H, W] views of the plans' logits buffers
        (k_l, k_u), (q_l, q_u) = self._beside(
            lambda: (cls2.forward_raw(z2[:L][1::2], no_backward=True), prj2.forward_raw(z2[L:], no_backward=True)),
            lambda: (cls1.forward_raw(z1[:L][0::2]), prj1.forward_raw(z1[L:])))
        ops.patch_nce(q_l, k_l, self.out_cl, dfeat=cls1.logits_grad_buffer(), temperature=self.temperature,
                      grad_scale=s["contrastive"])
        ops.patch_nce(q_u, k_u, self.out_cu, dfeat=prj1.logits_grad_buffer(), temperature=self.temperature,
                      grad_scale=s["contrastive"])
        cls1.backward_raw()
        prj1.backward_raw()
        ops.contrastive_cross_tail(o1, o2, lab, L, self.out1, dlogits=self.model1.logits_grad_buffer(),
                                   extra_l=cls1.input_grad_buffer(), extra_u=prj1.input_grad_buffer(),
                                   sup_scale=s["sup"], pseudo_scale=s["pseudo"], extra_scale=1.0, state=self.state)
        ops.contrastive_cross_tail(o2, o1, lab, L, self.out2, dlogits=self.model2.logits_grad_buffer(),
                                   sup_scale=s["sup"], pseudo_scale=s["pseudo"], state=self.state)
        scales = self._backward_pair(side=1)
        self._finish_step((self.model1, self.mom1, None, scales[0]), (self.model2, self.mom2, None, scales[1]))

    def losses(self):
        """Host copies of the last step's scalars: the quantities the reference logs (:286-294) and the terms behind them.
        ``lr`` is the rate the next step runs with, as the script logs ``lr_`` after computing it."""
        a, b, cl, cu = self.out1.cpu(), self.out2.cpu(), self.out_cl.cpu(), self.out_cu.cpu()
        c_l, c_u = cl[0].item(), cu[0].item()
        con = c_l + c_u
        return dict(loss=a[0].item() + b[0].item() + self.SCALES["contrastive"] * con,
                    model1_loss=a[5].item(), model2_loss=b[5].item(), con_loss=con, c_loss_l=c_l, c_loss_u=c_u,
                    consistency_weight=a[4].item(), lr=ops.read_step_state(self.state)["lr"],
                    loss1_ce=a[1].item(), loss1_dice=a[2].item(), pseudo_supervision1=a[3].item(),
                    loss2_ce=b[1].item(), loss2_dice=b[2].item(), pseudo_supervision2=b[3].item())


def linear_rampup(current, rampup_length):
    """reference code/utils/ramps.py:49-55"""
    assert current >= 0 and rampup_length >= 0
    return 1.0 if current >= rampup_length else current / rampup_length


class CnnMeetVitTrainer(_Step):
    """CNN student + Transformer student + EMA Transformer teacher (reference code/train_cnn_meet_vit_2D.py:293-352).

    ``model1`` (CNN) and ``model2`` (SwinUnet) see the whole batch and cross-teach through Dice on each other's
    arg-max pseudo labels with weight ``7 * consistency * linear_rampup(iter_num // 150, rampup)`` (:322-323,
    :336-337); both are also pulled towards ``ema_model`` -- the EMA of ``model2`` (:345), fed the noised unlabeled
    half (:298-309) -- by a softmax-MSE term with weight ``consistency * linear_rampup(...)`` that is zero while
    ``iter_num < 1000`` (:326-333).  ``loss = model1_loss + model2_loss``, two SGD steps, learning rate computed
    before ``iter_num`` is incremented (:347-348).  The two ramp weights are host floats of ``iter_num`` (no host
    sync: ``iter_num`` is the trainer's own counter)."""

    TRAIN_MODE = "train_cnn_meet_vit runs all three networks in train mode"

    def __init__(self, model1, model2, ema_model, *, labeled_bs, num_classes, base_lr=0.01, max_iterations=30000,
                 ema_decay=0.99, consistency=0.1, consistency_rampup=200.0, seed=1337, iter_num=0, momentum=0.9,
                 weight_decay=1e-4, process_group=None, use_tape=None):
        if model2.flat_param.numel() != ema_model.flat_param.numel():
            raise RuntimeError("the teacher is the EMA of model2: same architecture required")
        self._tape_weights = None
        self.model1, self.model2, self.ema_model = model1, model2, ema_model
        self._setup((model1, model2), (ema_model,), (1, 2, 3), labeled_bs=labeled_bs, num_classes=num_classes,
                    base_lr=base_lr, max_iterations=max_iterations, ema_decay=ema_decay, consistency=consistency,
                    consistency_rampup=consistency_rampup, cons_start_iter=1000, seed=seed, iter_num=iter_num,
                    momentum=momentum, weight_decay=weight_decay, process_group=process_group, use_tape=use_tape)
        # model1 is the side-stream student (_backward_pair): its tail bucket is deferred
        self._bucketers = (make_bucketer(model1, process_group, defer_tail=TWO_STREAM),
                           make_bucketer(model2, process_group))

    def weights(self):
        """(pseudo-supervision weight, mean-teacher weight) of the current iteration"""
        h = self.hyper
        w = h["consistency"] * linear_rampup(self.iter_num // h["ramp_div"], h["rampup"])
        return 7 * w, (w if self.iter_num >= h["cons_start_iter"] else 0.0)

    def step(self, volume_batch, label_batch, noise=None):
        return self._step(volume_batch, label_batch, noise)

    def _replay(self, volume, label, noise):
        # the two ramp weights are HOST floats of iter_num and arguments of the loss tails: the tape is recorded again whenever
        # they change (every ramp_div = 150 iterations, and at iteration 1000)
        if self.use_tape:
            w = self.weights()
            if self._tape is not None and w != self._tape_weights:
                self._tape, self._tape_warm = None, self.TAPE_WARMUP       # plans and buffers are warm: record at once
            if self._tape is None and self._tape_warm >= self.TAPE_WARMUP:
                self._tape_weights = w
        super()._replay(volume, label, noise)

    def _run(self, volume_batch, label_batch, noise):
        L = self.labeled_bs
        ema_in = self._noised(volume_batch[L:].contiguous(), noise)
        fwd1 = lambda: self.model1.forward_raw(volume_batch)
        fwd2 = lambda: self.model2.forward_raw(volume_batch)
        teacher = lambda: self.ema_model.forward_raw(ema_in, no_backward=True)
        if TWO_STREAM:
            # three independent forwards: the CNN student and the (half-batch) teacher beside the Transformer student --
            # roughly equal work; later the CNN's backward beside the Transformer's
            (o1, t), o2 = self._beside(lambda: (fwd1(), teacher()), fwd2)
        else:
            o1, o2, t = fwd1(), fwd2(), teacher()       # on one stream this step keeps the order of its networks
        lab = label_batch[:L].contiguous()
        w_cps, w_mt = self.weights()
        ops.cross_teaching_tail(o1, o2, lab, L, self.out1, dlogits=self.model1.logits_grad_buffer(),
                                cons_weight=w_cps, teacher=t, mt_weight=w_mt)
        ops.cross_teaching_tail(o2, o1, lab, L, self.out2, dlogits=self.model2.logits_grad_buffer(),
                                cons_weight=w_cps, teacher=t, mt_weight=w_mt)
        if TWO_STREAM:
            scales = self._backward_pair(side=0)
        else:
            # on one stream each student's exchange is finished before the other's backward begins (cross teaching keeps
            # both in flight instead): begin1, backward1, finish1, begin2, backward2, finish2
            scales = [backward_and_sync(m, self.pg, b) for m, b in zip(self._students, self._bucketers)]
        self._finish_step((self.model1, self.mom1, None, scales[0]),
                          (self.model2, self.mom2, self.ema_model.flat_param, scales[1]))

    def losses(self):
        a, b, d = self._pair_losses()
        d.update(consistency_loss1=a[5].item(), consistency_loss2=b[5].item(),
                 consistency_weight=a[4].item() / 7.0, mt_weight=a[6].item())
        return d


def triple_split(batch_size, labeled_bs):
    """U = batch_size - labeled_bs, the unlabeled samples of a triple-view step.  ValueError unless
    1 <= labeled_bs < batch_size: CE / Dice need a labeled sample, the six pseudo-label terms an unlabeled one."""
    B, L = int(batch_size), int(labeled_bs)
    if not 1 <= L < B:
        raise ValueError(f"triple-view training needs 1 <= labeled_bs < batch_size; got batch_size={B}, labeled_bs={L}")
    return B - L


class TripleViewTrainer(_Step):
    """Triple-view training (reference code/train_tripleview_2D(demo).py:290-354): three students see the whole batch, each
    is supervised on the labeled half and, on the unlabeled half, by the arg-max pseudo labels (Dice) of BOTH others;
    ``loss = model1_loss + model2_loss + model3_loss``, three SGD steps, no EMA, no noise, no ``iter_num < 1000`` gate.  The
    learning rate is computed before ``iter_num`` is incremented (:346-347).  The reference builds two ``net_factory``
    networks and a SwinUnet; any three networks of one ``num_classes`` and input shape do.

    One joint loss tail (``mis_triple_view_tail``) serves the three students: the pseudo labels are detached, so each
    student's logits gradient is that of its own loss.  model3 runs on the main stream, model1 then model2 beside it on
    the side stream, forward and backward.  With a process group the three flat gradient buffers are exchanged by three
    blocking all-reduces after the backwards: this trainer does not overlap the exchange with the backward."""

    TRAIN_MODE = "triple-view training trains all three networks (train mode)"

    def __init__(self, model1, model2, model3, *, labeled_bs, num_classes, base_lr=0.01, max_iterations=30000,
                 consistency=0.1, consistency_rampup=200.0, seed=1337, iter_num=0, momentum=0.9, weight_decay=1e-4,
                 process_group=None, use_tape=None):
        self.model1, self.model2, self.model3 = model1, model2, model3
        self._setup((model1, model2, model3), (), (1, 2, 3), labeled_bs=int(labeled_bs), num_classes=num_classes,
                    base_lr=base_lr, max_iterations=max_iterations, consistency=consistency,
                    consistency_rampup=consistency_rampup, lr_post_increment=True, seed=seed, iter_num=iter_num,
                    momentum=momentum, weight_decay=weight_decay, process_group=process_group, use_tape=use_tape)

    def step(self, volume_batch, label_batch):
        """One iteration on device tensors [B, 1, H, W] / [B, H, W]; returns the three device scalar buffers ``[loss_m,
        loss_ce, loss_dice, pseudo_supervision_a, consistency_weight, pseudo_supervision_b, ...]`` (no host sync)."""
        if volume_batch.dim() != 4 or label_batch.dim() != 3:
            raise ValueError(f"triple-view training runs the 2-D networks on [B, C, H, W] / [B, H, W]; got "
                             f"{tuple(volume_batch.shape)} / {tuple(label_batch.shape)}")
        triple_split(volume_batch.shape[0], self.labeled_bs)
        return self._step(volume_batch, label_batch)

    def _run(self, volume_batch, label_batch):
        L = self.labeled_bs
        nets = self._students
        fwd = [lambda net=net: net.forward_raw(volume_batch) for net in nets]
        if TWO_STREAM:
            # the students only meet in the loss tail: model1 then model2 beside model3
            (o1, o2), o3 = self._beside(lambda: (fwd[0](), fwd[1]()), fwd[2])
        else:
            o1, o2, o3 = fwd[0](), fwd[1](), fwd[2]()       # on one stream this step keeps the order of its networks
        ops.triple_view_tail(o1, o2, o3, label_batch[:L].contiguous(), L, (self.out1, self.out2, self.out3),
                             dlogits=[net.logits_grad_buffer() for net in nets], state=self.state)
        self._backward_beside(side=(0, 1), main=(2,))
        scales = [_lib.tape_call(dist.sync_gradients, net.flat_grad, self.pg) for net in nets]
        self._finish_step(*((net, mom, None, scale)
                            for net, mom, scale in zip(nets, (self.mom1, self.mom2, self.mom3), scales)))

    def losses(self):
        """Host copies of the last step's scalars (three small D2H)."""
        d = {}
        for m, out in enumerate((self.out1, self.out2, self.out3), start=1):
            o = out.cpu()
            d.update({f"model{m}_loss": o[0].item(), f"loss{m}_ce": o[1].item(), f"loss{m}_dice": o[2].item(),
                      f"pseudo_supervision{m}a": o[3].item(), f"pseudo_supervision{m}b": o[5].item(),
                      "consistency_weight": o[4].item()})
        d["loss"] = d["model1_loss"] + d["model2_loss"] + d["model3_loss"]
        return d


class AdversarialTrainer(_Step):
    """Adversarial network training (reference code/train_adversarial_network_3D.py:129-175 with FC3DDiscriminator,
    code/train_adversarial_network_2D.py with networks.discriminator_2d.FCDiscriminator: the discriminator is whichever object
    is handed in, the batch follows ``model.ndim_spatial``), two phases per step, both recorded on the launch tape:

    A (segmenter)      student forward in train mode; the discriminator, frozen and in eval mode (no dropout), judges
                       softmax(outputs[L:]) against the target 1 and hands back its cross-entropy and the gradient at
                       its ``map`` input -- no parameter gradient is formed, the reference discards it; one fused tail
                       (``mis_adversarial_tail``) writes 0.5 * (CE + Dice) + w * consistency_loss and the logits gradient;
                       student backward, SGD (momentum 0.9, wd 1e-4).
    B (discriminator)  student forward in eval mode with the weights phase A just updated (no backward, on a plan of
                       its own); the discriminator in train mode (Dropout3d from the step's Philox state) on all B
                       samples against the target ``1 if i < labeled_bs else 0``; its backward; Adam (``dan_lr``,
                       betas (0.9, 0.99)) with the step count on the device.

    Then the schedule: poly LR and w = consistency * sigmoid_rampup(iter_num // 150, rampup) in the Mean-Teacher order.
    The student's softmax is never written: the discriminator's first layer reads the logits through it.  Single process:
    the discriminator's gradient has no exchange."""

    TRAIN_MODE = "the adversarial step switches train / eval mode itself: hand it both networks in train mode"

    def __init__(self, model, dan, *, labeled_bs, num_classes, base_lr=0.01, dan_lr=1e-4, max_iterations=30000,
                 consistency=0.1, consistency_rampup=200.0, seed=1337, iter_num=0, momentum=0.9, weight_decay=1e-4,
                 betas=(0.9, 0.99), eps=1e-8, process_group=None, use_tape=None):
        if dist.world_size(process_group) > 1:
            raise NotImplementedError("AdversarialTrainer is single-process: the discriminator's gradient is not exchanged")
        if not 0 < int(labeled_bs):
            raise ValueError(f"adversarial training needs labeled samples, got labeled_bs={labeled_bs}")
        self.model, self.dan = model, dan
        self._setup((model,), (dan,), (1, 2), labeled_bs=int(labeled_bs), num_classes=num_classes, base_lr=base_lr,
                    max_iterations=max_iterations, consistency=consistency, consistency_rampup=consistency_rampup,
                    seed=seed, iter_num=iter_num, momentum=momentum, weight_decay=weight_decay,
                    process_group=process_group, use_tape=use_tape)
        self.dan_lr, self.betas, self.eps = float(dan_lr), (float(betas[0]), float(betas[1])), float(eps)
        self.adam_m, self.adam_v = torch.zeros_like(dan.flat_param), torch.zeros_like(dan.flat_param)
        self.adam_state = torch.zeros(2, dtype=torch.int64, device="cuda")
        ops.adam_init(self.adam_state, 0)
        self.dan_out = torch.zeros(1, dtype=torch.float32, device="cuda")
        self._targets = {}

    def _target(self, B, ones):
        """int32 [B]: phase B's ``1 if i < labeled_bs else 0``; ``ones``: phase A's all-ones target of the unlabeled samples."""
        t = self._targets.get((B, ones))
        if t is None:
            t = (torch.ones(B) if ones else (torch.arange(B) < self.labeled_bs)).to(torch.int32).cuda()
            self._targets[(B, ones)] = t
        return t

    def _run(self, volume, label):
        L, m, dan = self.labeled_bs, self.model, self.dan
        B = volume.shape[0]
        # ---- phase A
        dan.eval()
        s_logits = m.forward_raw(volume)
        self.pass_a = m.last_pass()              # phase B's forward runs on a plan of its own: this pass stays readable
        dan.loss_forward(s_logits[L:], volume[L:], self._target(B - L, True))
        dan.loss_backward(params=False, dmap=True)
        ops.adversarial_tail(s_logits, label[:L].contiguous(), L, dan.dmap_buffer(), dan.loss_buffer(), self.out,
                             dlogits=m.logits_grad_buffer(), state=self.state)
        grad_scale = backward_and_sync(m, self.pg)
        ops.sgd_ema_step(m.flat_param, m.flat_grad, self.momentum_buf, None, momentum=self.momentum,
                         weight_decay=self.weight_decay, grad_scale=grad_scale, state=self.state)
        # ---- phase B
        m.eval()
        b_logits = m.forward_raw(volume, no_backward=True, slot=1)
        m.train()
        dan.train()
        dan.loss_forward(b_logits, volume, self._target(B, False))
        dan.loss_backward(params=True, dmap=False)
        self.dan_out = dan.loss_buffer()             # static per batch shape: the recorded launches write it again
        ops.adam_step(dan.flat_param, dan.flat_grad, self.adam_m, self.adam_v, self.adam_state, self.dan_lr, self.betas,
                      self.eps)
        self._advance_schedule()

    def step(self, volume_batch, label_batch):
        """One iteration on device tensors [B, 1, D, H, W] / [B, D, H, W] (a 2-D model: [B, 1, H, W] / [B, H, W]); returns the device scalar buffer ``[loss, loss_ce,
        loss_dice, consistency_loss, consistency_weight, ...]`` (no host sync); ``dan_out[0]`` is the discriminator's loss."""
        nd = 2 + self.model.ndim_spatial
        if volume_batch.dim() != nd:
            raise ValueError(f"adversarial training of a {self.model.ndim_spatial}-D network runs on "
                             f"{'[B, C, D, H, W]' if nd == 5 else '[B, C, H, W]'}; got {tuple(volume_batch.shape)}")
        if not self.labeled_bs < volume_batch.shape[0]:
            raise ValueError(f"adversarial training needs unlabeled samples: batch {volume_batch.shape[0]}, "
                             f"labeled_bs {self.labeled_bs}")
        return self._step(volume_batch, label_batch)

    def losses(self):
        o = self.out.cpu()
        return dict(loss=o[0].item(), loss_ce=o[1].item(), loss_dice=o[2].item(), consistency_loss=o[3].item(),
                    consistency_weight=o[4].item(), DAN_loss=self.dan_out.item())

    # ---- checkpoint: the discriminator and its optimizer
    def dan_checkpoint(self):
        return dict(state_dict={k: v.detach().cpu().clone() for k, v in self.dan.state_dict().items()},
                    adam_m=self.adam_m.cpu(), adam_v=self.adam_v.cpu(), adam_step=int(self.adam_state[0].item()))

    def load_dan_checkpoint(self, ck):
        self.dan.load_state_dict(ck["state_dict"])
        self.adam_m.copy_(ck["adam_m"])
        self.adam_v.copy_(ck["adam_v"])
        ops.adam_init(self.adam_state, int(ck["adam_step"]))
