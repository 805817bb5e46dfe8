"""Mean-teacher semi-supervised train step (Tarvainen & Valpola 2017; UA-MT: Yu et al., MICCAI 2019) for the MI355X UNet path.

The reference's `SemiTrainer` is a supervised loop; this is the project's own addition.  A batch holds `labeled_bs` labelled
images followed by unlabelled ones.  The student is trained with `supervised_loss` on the labelled part plus a softmax-MSE
consistency term (`losses.consistency_loss.SoftmaxMSEConsistency`, csrc/consistency.hip) that pulls its logits on the unlabelled
part towards those of a teacher -- a second network of the same architecture whose weights are the exponential moving average of
the student's (`ops.ema_update`: ONE pass over `FlatOptimizer.flat_param`).  With `uncertainty_passes = T > 0` the term is masked
by the entropy of the mean of T stochastic teacher passes (fresh input noise, fresh Dropout2d masks), accumulated by the
prediction path's `mia_softmax_accum`.

The engines of this file derive from `SemiEngine`, which owns what they share on top of `training.engine.EngineBase`: the
batch convention and its checks, the schedule buffer `dyn` and the skeleton of `train_step`.  An engine adds its networks, its loss
and what it does after the optimizer step; `TrainEngine` is not involved.

Out of scope:
* hipGraph capture of this step: it runs eagerly.  The consistency weight and the entropy threshold already live in a device
  buffer (`dyn`) that the kernels read when they run, so a capture can follow later.
* more than one rank: the constructor raises `NotImplementedError`.
* 3-D inputs; deep supervision in `MeanTeacherEngine` (the one-network case is `URPCEngine` below).

`URPCEngine` is the one-network method of the same tables (URPC: Luo et al., MICCAI 2021 / MedIA 2022): no teacher and no extra
passes.  The network's own multi-scale outputs (`UNet(deep_supervision=True, ds_layer=n)`) are all supervised on the labelled images
and asked to agree on the unlabelled ones (`losses.pyramid_consistency.PyramidConsistencyLoss`, csrc/urpc.hip).  Same batch
convention, same device-resident schedule buffer `dyn`; it runs eagerly on one rank on 2-D inputs, with index labels.

`CPSEngine` is cross pseudo supervision (CPS: Chen et al., CVPR 2021), the two-network row of those tables: two networks of different
initialisation, both trained, each on the supervised loss plus cross-entropy on the other's hard pseudo-labels
(`losses.cross_pseudo.CrossPseudoSupervisionLoss`, csrc/cps.hip).  One `backward()` feeds two `FlatOptimizer`s.  Same batch
convention and `dyn = {weight, confidence threshold}`; eager, one rank, 2-D inputs.  `cutmix=True` is the CutMix form, on the
weak-to-strong kernels described below.  Out of scope: Dice on pseudo-labels.

`VATEngine` is virtual adversarial training (VAT: Miyato et al., TPAMI 2018), the one semi-supervised method the reference itself ships
(`losses/adv_loss.py`): one network, no teacher.  The unlabelled images are pushed `eps` along the direction that changes the
network's own prediction most -- found by a power iteration on the gradient of a KL distance with respect to the IMAGE
(`losses.vat_loss.VATLoss`, csrc/vat.hip, csrc/stem_dgrad.hip) -- and the network is asked to predict there what it predicts on the
clean image.  Same batch convention, `dyn = {weight, eps}`; eager, one rank, 2-D inputs.

`BCPEngine` is bidirectional copy-paste (BCP: Bai et al., CVPR 2023), the one method of those tables that mixes labelled and unlabelled
images: a box of a labelled image is pasted into an unlabelled one and the other way round (`ops.bcp_mix`), and every pixel of a mixed
image is supervised by the ground truth or by the EMA teacher's pseudo-label, whichever image it came from
(`losses.copy_paste.CopyPasteLoss`, csrc/bcp.hip).  It shares the teacher machinery (`_EMATeacher`) with `MeanTeacherEngine`.  Eager,
one rank, 2-D inputs, index labels.  Out of scope: 3-D volumes, per-image masks in the engine (the kernels take them).

`FixMatchEngine` is weak-to-strong consistency (FixMatch: Sohn et al., NeurIPS 2020; with two strong views the dual-stream perturbation
of UniMatch: Yang et al., CVPR 2023): one network and no teacher.  The network predicts on the unlabelled images as they come (the
weak view); its confident arg-max labels (`ops.w2s_labels`) supervise the SAME network on strongly augmented views of those images
that are CutMix-ed with a permutation of themselves (`ops.cutmix_perm`), where a pixel under a box takes the pseudo-label of the image
it came from (`losses.weak_strong.WeakToStrongLoss`, csrc/w2s.hip).  Same batch convention, `dyn = {u_weight, confidence threshold}`;
eager, one rank, 2-D inputs.  As in FixMatch's published code the labelled and the strong rows share one forward, and with batch norm
its statistics.  Where it departs from the published code: the weak view, which shares that forward there, has a gradient-free pass
of its own here that leaves the running statistics alone (`ops.no_bn_tracking`; two forwards of one network before a backward would
break the hint mechanism, so the weak pass comes first); the images of the batch ARE the weak view (the geometric augmentation
happens upstream); the CutMix partner is a permutation of the unlabelled half of the SAME batch where UniMatch draws a second
unlabelled batch from the loader; the mix is a selection, not a blend; the box aspect is drawn from the part of the range that fits
instead of redrawn until it does; the CE denominator is always the pixel count, where UniMatch divides by the kept pixels.  Out of
scope: UniMatch's feature-perturbation stream (Dropout2d on the skips between encoder and decoder), graph capture, more than one
rank, 3-D.

`DTCEngine` is dual-task consistency (DTC: Luo et al., AAAI 2021): one network with TWO 1x1 heads on the last decoder activation
(`models.unet.DualTaskUNet`), the segmentation logits and a level-set map -- `tanh` of a regression of the normalised signed distance
to the object boundary.  On the labelled images the level-set head regresses the target that `signed_distance_map` and
`ops.sdm_extent` give from the labels the step sees; on EVERY image `sigmoid(-1500 tanh)` of the level-set head must agree with the
soft-max of the segmentation head (`losses.dual_task.DualTaskConsistencyLoss`, csrc/dtc.hip).  No teacher, no extra pass: one
training forward of the whole batch.  Same batch convention; `dyn = {consistency weight, beta}`; eager, one rank, 2-D inputs, index
labels.  Out of scope: 3-D, graph capture, a pixel spacing other than 1, a level-set head on a subset of the classes.
"""
from __future__ import annotations

import math
from pathlib import Path
from typing import Optional

import torch
import torch.distributed as dist

from mia_hip import ops
from training.engine import EngineBase

TEACHER_FILE = "mean_teacher.pth"
CPS_PEER_FILE = "cps_peer.pth"


def ema_alpha(step: int, ema_decay: float) -> float:
    """The published schedule: `min(1 - 1 / (step + 1), ema_decay)` with `step` the number of EMA updates done so far -- the first
    update copies the student (alpha = 0), the early ones average quickly, later ones use `ema_decay`."""
    return min(1.0 - 1.0 / (step + 1), float(ema_decay))


def entropy_threshold(ramp: float, num_classes: int) -> float:
    """UA-MT's threshold `(0.75 + 0.25 * ramp) * ln(K)` for K classes (background included) and a ramp value in [0, 1]."""
    return (0.75 + 0.25 * float(ramp)) * math.log(num_classes)


def _ramp_value(r, i: int) -> float:
    """A float, or any object with `.step(i)` (the reference's `scheduler.ramps.BaseRampUp` protocol)."""
    return float(r.step(i)) if hasattr(r, "step") else float(r)


class SemiEngine(EngineBase):
    """The part of a semi-supervised engine that does not depend on the method.  A batch is {"image": [B,C,H,W], "label":
    [>= labeled_bs, H, W]}: the first `labeled_bs` images are the labelled ones.  `train_step` is the common skeleton; a subclass gives
    `_loss(image, label)` (forward passes and loss terms; it calls `_write_dyn` before anything reads `dyn`, and only when it forms the
    unsupervised term), `_dyn_values()` and, where it has them, `_nets()`, `_steppers()` and `_after_step()`.

    `dyn` is the device buffer of the values that follow a schedule, read by the loss kernels when they run: dyn[0] is the weight of
    the unsupervised term, dyn[1] the method's threshold (unused by URPC)."""

    _one_rank_why = ""

    def __init__(self, model, labeled_bs: int, grad_norm: float, process_group, *optimizer_args):
        """optimizer_args: (optimizer_name, optimizer_kwargs, start_lr, num_iters, lr_warmup_iter, lr_interval, lr_scheduler_name)."""
        who = type(self).__name__
        if dist.is_initialized() and dist.get_world_size(process_group) > 1:
            raise NotImplementedError(f"{who} runs on one rank{self._one_rank_why}")
        if labeled_bs < 1:
            raise ValueError(f"{who}: labeled_bs must be at least 1")
        self.model = model
        self.labeled_bs = int(labeled_bs)
        self._optimizer_args = optimizer_args
        self.optimizer, self.lr_scheduler = self._make_optimizer(model, *optimizer_args)
        self.grad_norm = grad_norm
        self.dyn = torch.zeros(2, device=self.optimizer.flat_param.device, dtype=torch.float32)
        self.current_iter = 0

    def _nets(self):
        """The networks `train_step` puts into train mode."""
        return (self.model,)

    def _steppers(self):
        """(optimizer, LR scheduler or None) of every trained network, in the order they step."""
        return ((self.optimizer, self.lr_scheduler),)

    def _after_step(self) -> None:
        """What follows the optimizer step(s)."""

    def _write_dyn(self) -> None:
        for slot, v in enumerate(self._dyn_values()):
            self.dyn[slot].fill_(v)  # a fill launch that carries the value as an argument: no staging copy, no host sync

    def _stage(self, sampled_batch):
        who = type(self).__name__
        dev = self.optimizer.flat_param.device
        lb = self.labeled_bs
        image = sampled_batch["image"].to(dev, dtype=torch.float32, non_blocking=True)
        label = sampled_batch["label"].to(dev, non_blocking=True)
        if image.ndim != 4:
            raise NotImplementedError(f"{who} implements 2-D inputs [B, C, H, W]")
        if label.shape[0] < lb or image.shape[0] < lb:
            raise ValueError(f"{who}: {label.shape[0]} label maps / {image.shape[0]} images for labeled_bs={lb}")
        return image, label

    def train_step(self, sampled_batch) -> torch.Tensor:
        """{"image": [B,C,H,W], "label": [>= labeled_bs, H, W]}: the first `labeled_bs` images are the labelled ones."""
        for net in self._nets():
            net.train()
        steppers = self._steppers()
        for _, sched in steppers:
            if sched:
                sched.step(self.current_iter)
        loss = self._loss(*self._stage(sampled_batch))
        for opt, _ in steppers:
            opt.zero_grad()
        self._backward(loss)
        for opt, _ in steppers:
            opt.step(max_grad_norm=self.grad_norm)
        self._after_step()
        self.current_iter += 1
        return loss.detach()


class _EMATeacher:
    """What the engines with an EMA teacher share (`MeanTeacherEngine`, `BCPEngine`), mixed in beside `SemiEngine`: the teacher's
    parameters as views into `teacher_flat`, the EMA + re-pack after the optimizer step, prediction with either network, and the
    teacher's file in a checkpoint.  The engine sets `self.teacher` and `self.ema_decay`, then calls `_init_teacher()`."""

    def _init_teacher(self) -> None:
        self._adopt_teacher()
        self.ema_step = 0
        self._teacher_plan = None

    def _nets(self):
        return (self.model, self.teacher)

    def _adopt_teacher(self) -> None:
        """Teacher parameters -> views into `teacher_flat` at the student's offsets; values and buffers copied from the student."""
        opt = self.optimizer
        names = {id(p): n for n, p in self.model.named_parameters()}
        tparams = dict(self.teacher.named_parameters())
        if set(tparams) != set(names.values()) or any(tparams[names[id(p)]].shape != p.shape for p in opt.params):
            raise ValueError(f"{type(self).__name__}: the teacher must have the student's architecture (same parameter names and shapes)")
        self.teacher.to(opt.flat_param.device)
        self.teacher.load_state_dict(self.model.state_dict())  # buffers and frozen parameters; the trainable ones again below
        self.teacher_flat = torch.zeros_like(opt.flat_param)
        self.teacher_params = []
        with torch.no_grad():
            self.teacher_flat.copy_(opt.flat_param)
            for p, o in zip(opt.params, opt.offsets):
                t = tparams[names[id(p)]]
                t.data = self.teacher_flat[o:o + p.numel()].view(p.shape)
                t.requires_grad_(False)
                t.grad = None
                self.teacher_params.append(t)
        for t in self.teacher.parameters():
            t.requires_grad_(False)
        ops.bump_param_epoch()

    def _after_step(self) -> None:
        """The EMA over the flat buffers, then the teacher's packed weight copies.  The optimizer step just before has moved the
        parameter epoch on, so every packed copy of a teacher weight made before this point misses on its next use; the plan
        re-packs them in one launch and marks them current.  The decay follows `ema_step`, the number of EMA updates done so far,
        not `current_iter`."""
        ops.ema_update(self.teacher_flat, self.optimizer.flat_param, ema_alpha(self.ema_step, self.ema_decay))
        self.ema_step += 1
        if self.ema_step < 2 or not self.teacher_flat.is_cuda:
            return
        if self._teacher_plan is None or not self._teacher_plan.valid():
            dts = set()
            for t in self.teacher_params:
                c = ops._caches.get(id(t))
                if c is not None and c[0]() is t:
                    dts.update(dt for dt, _ in c[1]._store)
            if len(dts) != 1:  # nothing packed yet (no teacher pass so far), or mixed compute dtypes: the per-tensor path
                return
            self._teacher_plan = ops.PackPlan(self.teacher_params, dts.pop())
        self._teacher_plan.repack()

    def predict(self, image: torch.Tensor, use_teacher: bool = False) -> torch.Tensor:
        """eval forward -> softmax -> argmax, with the student's or the teacher's weights."""
        return self._predict(self.teacher if use_teacher else self.model, image)

    def save_state_dict(self, save_path, save_training_state: bool = False, **extra) -> None:
        """The student as `TrainEngine.save_state_dict` writes it (model.pth, training_state.pth on request: the reference's
        layout), plus the teacher's `state_dict` and the EMA step count in a file of their own."""
        from training import checkpoint
        super().save_state_dict(save_path, save_training_state, **extra)
        torch.save({"teacher": checkpoint.model_state_for_save(self.teacher), "ema_step": int(self.ema_step)},
                   Path(save_path) / TEACHER_FILE)

    def load_state_dict(self, save_path) -> dict:
        out = super().load_state_dict(save_path)
        tf = Path(save_path) / TEACHER_FILE
        if tf.is_file():
            sd = torch.load(tf, map_location=self.teacher_flat.device, weights_only=True)
            self.teacher.load_state_dict(sd["teacher"])  # copy_ into the flat-buffer views
            self.ema_step = int(sd["ema_step"])
        ops.bump_param_epoch()  # packed weights of both networks are stale now
        return out


class MeanTeacherEngine(_EMATeacher, SemiEngine):
    """student + EMA teacher + supervised loss + consistency loss + flat optimizer + poly LR.  `train_step` returns the loss TENSOR
    (no host sync); `last_supervised`, `last_consistency` (unweighted) and `last_kept` are device by-products of the latest step.

    teacher: a second `UNet` of the student's architecture.  Its trainable parameters become views into `teacher_flat`, a buffer
    with the student's `FlatOptimizer` offsets, initialised bit for bit from the student; they never receive a gradient.  The teacher
    stays in train mode during training (its Dropout2d masks are what makes the uncertainty passes stochastic, as in the published
    code).
    consistency: None = `SoftmaxMSEConsistency` for the student's classes; a module with that call signature; False = no teacher
    pass and no consistency term (the EMA still runs).
    consistency_weight, threshold_ramp: a float or an object with `.step(i)`; each step the engine writes
    `weight_i` and `threshold_i = (0.75 + 0.25 * ramp_i) * ln(K)` into the device buffer `dyn` before anything reads it, outside
    the autograd graph.  threshold_ramp None = 0, i.e. the schedule's strictest threshold `0.75 ln K` throughout.
    uncertainty_passes: T extra teacher passes whose mean soft-max masks the consistency term; 0 = the plain Mean Teacher form.
    noise_std, noise_clip: the teacher sees `image + clamp(N(0, noise_std^2), -noise_clip, noise_clip)`."""

    _one_rank_why = " (the EMA and the teacher passes are not sharded yet)"

    def __init__(self, model, teacher, supervised_loss, labeled_bs: int, ema_decay: float = 0.99, consistency=None,
                 consistency_weight=0.1, uncertainty_passes: int = 0, threshold_ramp=None, noise_std: float = 0.1,
                 noise_clip: float = 0.2, optimizer_name: str = "adam", optimizer_kwargs: Optional[dict] = None,
                 start_lr: float = 1e-3, num_iters: int = 4000, lr_warmup_iter: int = 250, lr_interval: int = 1,
                 lr_scheduler_name: str = "poly", grad_norm: float = 10.0, process_group=None):
        if not 0.0 <= ema_decay <= 1.0:
            raise ValueError("MeanTeacherEngine: ema_decay must lie in [0, 1]")
        if uncertainty_passes < 0:
            raise ValueError("MeanTeacherEngine: uncertainty_passes must not be negative")
        super().__init__(model, labeled_bs, grad_norm, process_group, optimizer_name, optimizer_kwargs, start_lr, num_iters,
                         lr_warmup_iter, lr_interval, lr_scheduler_name)
        self.teacher = teacher
        self.supervised_loss = supervised_loss
        self.ema_decay = float(ema_decay)
        self.uncertainty_passes = int(uncertainty_passes)
        self.consistency_weight, self.threshold_ramp = consistency_weight, threshold_ramp
        self.noise_std, self.noise_clip = float(noise_std), float(noise_clip)
        self.num_classes = int(model.decoder.seg_output.weight.shape[0])  # K: background included
        if consistency is None:
            from losses.consistency_loss import SoftmaxMSEConsistency
            consistency = SoftmaxMSEConsistency(self.num_classes - 1)
        self.consistency = consistency or None
        self._init_teacher()
        self.last_supervised = self.last_consistency = self.last_kept = None

    def _dyn_values(self):
        r = 0.0 if self.threshold_ramp is None else _ramp_value(self.threshold_ramp, self.current_iter)
        return _ramp_value(self.consistency_weight, self.current_iter), entropy_threshold(r, self.num_classes)

    def _noisy(self, x: torch.Tensor) -> torch.Tensor:
        if self.noise_std == 0.0:
            return x
        return x + torch.clamp(torch.randn_like(x) * self.noise_std, -self.noise_clip, self.noise_clip)

    @torch.no_grad()
    def _teacher_passes(self, unlabeled: torch.Tensor):
        """(zt, pbar): the teacher's logits on one noisy copy, and the mean soft-max of `uncertainty_passes` further stochastic passes
        (None without them).  Runs BEFORE the student's forward: `UNet.forward` clears the producer -> consumer hints that belong to
        the backward of the latest forward."""
        zt = self.teacher(self._noisy(unlabeled))
        pbar = None
        if self.uncertainty_passes > 0:
            from inference.predictor import softmax_accum
            pbar = torch.empty(zt.shape, device=zt.device, dtype=torch.float32)
            for i in range(self.uncertainty_passes):
                softmax_accum(self.teacher(self._noisy(unlabeled)), pbar, None, weight=1.0 / self.uncertainty_passes, first=i == 0)
        return zt, pbar

    def _loss(self, image: torch.Tensor, label: torch.Tensor) -> torch.Tensor:
        lb = self.labeled_bs
        consistent = self.consistency is not None and image.shape[0] > lb
        if consistent:
            self._write_dyn()
            zt, pbar = self._teacher_passes(image[lb:])
        output = self.model(image)
        sup = self.supervised_loss(output[:lb], label[:lb])
        self.last_supervised = sup.detach()
        if not consistent:
            return sup
        loss = sup + self.consistency(output[lb:], zt, pbar, dyn=self.dyn)
        self.last_consistency = getattr(self.consistency, "last_value", None)
        self.last_kept = getattr(self.consistency, "last_kept", None)
        return loss


class URPCEngine(SemiEngine):
    """one network + deep-supervised loss on the labelled images + pyramid consistency on the unlabelled ones + flat optimizer + poly
    LR.  `train_step` returns the loss TENSOR (no host sync); `last_supervised` and `last_consistency` (unweighted) are device
    by-products of the latest step.

    model: a `UNet` built with auxiliary heads (`deep_supervision=True, ds_layer >= 2`).  Per step
        outs = model(image, return_ds=True, upsample_ds=False)
        sup  = DeepSupervisionLoss(supervised_loss, weights=[1/S] * S)([o[:labeled_bs] for o in outs], label[:labeled_bs])
        cons = consistency([o[labeled_bs:] for o in outs], dyn=dyn)           skipped when the batch has no unlabelled image
    consistency: None = `PyramidConsistencyLoss()`; a module with that call signature; False = no consistency term.
    consistency_weight: a float or an object with `.step(i)`; each step the engine writes `weight_i` into the device buffer `dyn`
    before anything reads it, outside the autograd graph."""

    def __init__(self, model, supervised_loss, labeled_bs: int, consistency=None, consistency_weight=0.1,
                 optimizer_name: str = "adam", optimizer_kwargs: Optional[dict] = None, start_lr: float = 1e-3, num_iters: int = 4000,
                 lr_warmup_iter: int = 250, lr_interval: int = 1, lr_scheduler_name: str = "poly", grad_norm: float = 10.0,
                 process_group=None):
        heads = getattr(getattr(model, "decoder", None), "ds", None)
        if heads is None or all(h is None for h in heads):
            raise ValueError("URPCEngine needs a model whose decoder has auxiliary heads (UNet(deep_supervision=True, ds_layer >= 2)): "
                             "the consistency term compares their outputs")
        super().__init__(model, labeled_bs, grad_norm, process_group, optimizer_name, optimizer_kwargs, start_lr, num_iters,
                         lr_warmup_iter, lr_interval, lr_scheduler_name)
        self.num_outputs = 1 + sum(h is not None for h in heads)
        from losses.deep_supervision import DeepSupervisionLoss
        self.supervised_loss = DeepSupervisionLoss(supervised_loss, weights=[1.0 / self.num_outputs] * self.num_outputs)
        if consistency is None:
            from losses.pyramid_consistency import PyramidConsistencyLoss
            consistency = PyramidConsistencyLoss()
        self.consistency = consistency or None
        self.consistency_weight = consistency_weight
        self.last_supervised = self.last_consistency = None

    def _dyn_values(self):
        return (_ramp_value(self.consistency_weight, self.current_iter),)

    def _loss(self, image: torch.Tensor, label: torch.Tensor) -> torch.Tensor:
        lb = self.labeled_bs
        outs = self.model(image, return_ds=True, upsample_ds=False)
        sup = self.supervised_loss([o[:lb] for o in outs], label[:lb])
        self.last_supervised = sup.detach()
        if self.consistency is None or image.shape[0] <= lb:
            return sup
        self._write_dyn()  # after the forward here, before the teacher pass in MeanTeacherEngine: what counts is that it precedes the loss
        loss = sup + self.consistency([o[lb:] for o in outs], dyn=self.dyn)
        self.last_consistency = getattr(self.consistency, "last_value", None)
        return loss


class CPSEngine(SemiEngine):
    """two networks + supervised loss on the labelled images for each + cross pseudo supervision between them + two flat optimizers +
    two poly LR schedules.  `train_step` returns the loss TENSOR (no host sync); `last_supervised`, `last_cps` (the unweighted
    LA + LB), `last_agree` (int64: pixels of the CPS slice where the two arg-max labels agree) and `last_confident` (int64 [2]) are
    device by-products of the latest step.  Per step

        out_a = model_a(image);  out_b = model_b(image)
        sup   = supervised_loss(out_a[:lb], label[:lb]) + supervised_loss(out_b[:lb], label[:lb])
        s     = 0 if cps_on_labeled else lb        # the paper uses every image, SSL4MIS the unlabelled ones only
        loss  = sup + cps(out_a[s:], out_b[s:], dyn=dyn)      # skipped when that slice is empty
        one backward; clip and step each optimizer on its own

    model_a, model_b: two `UNet`s with the same class count and different initialisations (two objects: the same object twice is an
    error).  `self.model` / `self.optimizer` / `self.lr_scheduler` are network A's, so `training/checkpoint.py` serves it unchanged;
    network B's carry the suffix `_b`.
    cps_weight, confidence_threshold: a float or an object with `.step(i)`; each step the engine writes `weight_i` and `tau_i` into the
    device buffer `dyn` before anything reads it, outside the autograd graph.  tau = 0 (the default) is the published CPS; tau > 0
    lets a network learn only from labels whose source gives them a soft-max of at least tau.

    `cutmix=True` is the CutMix form of the paper: the pseudo-labels come from the CLEAN unlabelled images and the
    networks are trained on a CutMix of them.  With U = image[lb:], per step

        za = model_a(U);  zb = model_b(U)           no gradient, batch-norm running statistics untouched, BEFORE the training forwards
        code_a = ops.w2s_labels(za, dyn)[0];  code_b = ops.w2s_labels(zb, dyn)[0]
        mask = box_masks(random_cutmix_boxes(nu, H, W, cutmix_prob, cutmix_size, cutmix_ratio));  perm = torch.randperm(nu)
        net_in = [image[:lb]; ops.cutmix_perm(U, perm, mask)]             ONE input for both networks
        out_a = model_a(net_in);  out_b = model_b(net_in)
        loss  = sup + w2s(out_a[lb:], code_b, mask, perm, dyn=dyn) + w2s(out_b[lb:], code_a, mask, perm, dyn=dyn)

    with `w2s = WeakToStrongLoss(K - 1, ce_weight=1, dice_weight=0)` (csrc/w2s.hip): a pixel under a box is supervised by the OTHER
    network's label of the image it came from.  `last_cps` is then the unweighted sum of the two CE terms, `last_confident` the two
    networks' confident pixels on the clean images, `last_agree` None; `last_mask`, `last_perm`, `last_net_in` and `last_codes`
    (the two code maps) are further by-products.  The unlabelled images mix among themselves (the paper mixes two unlabelled batches); `cps_on_labeled` does not
    combine with it.  With `cutmix=False`, the default, not one launch differs from the plain form above."""

    def __init__(self, model_a, model_b, supervised_loss, labeled_bs: int, cps_weight=0.1, confidence_threshold=0.0,
                 cps_on_labeled: bool = False, optimizer_name: str = "adam", optimizer_kwargs: Optional[dict] = None,
                 start_lr: float = 1e-3, num_iters: int = 4000, lr_warmup_iter: int = 250, lr_interval: int = 1,
                 lr_scheduler_name: str = "poly", grad_norm: float = 10.0, process_group=None, cutmix: bool = False,
                 cutmix_prob: float = 1.0, cutmix_size=(0.02, 0.4), cutmix_ratio=(0.3, 1 / 0.3)):
        if model_a is model_b:
            raise ValueError("CPSEngine needs two networks: model_a and model_b are the same object")
        if cutmix and cps_on_labeled:
            raise ValueError("CPSEngine: cutmix=True mixes the unlabelled images only; cps_on_labeled does not combine with it")
        if not 0.0 <= cutmix_prob <= 1.0:
            raise ValueError("CPSEngine: cutmix_prob must lie in [0, 1]")
        ka, kb = (int(m.decoder.seg_output.weight.shape[0]) for m in (model_a, model_b))
        if ka != kb:
            raise ValueError(f"CPSEngine: the networks predict {ka} and {kb} classes")
        super().__init__(model_a, labeled_bs, grad_norm, process_group, optimizer_name, optimizer_kwargs, start_lr, num_iters,
                         lr_warmup_iter, lr_interval, lr_scheduler_name)
        self.model_b = model_b
        self.optimizer_b, self.lr_scheduler_b = self._make_optimizer(model_b, *self._optimizer_args)
        if self.optimizer.flat_param.device != self.optimizer_b.flat_param.device:
            raise ValueError("CPSEngine: the two networks live on different devices")
        self.supervised_loss = supervised_loss
        self.cps_weight, self.confidence_threshold = cps_weight, confidence_threshold
        self.cps_on_labeled = bool(cps_on_labeled)
        self.num_classes = ka  # K: background included
        from losses.cross_pseudo import CrossPseudoSupervisionLoss
        self.cps = CrossPseudoSupervisionLoss(self.num_classes - 1)
        self.cutmix = bool(cutmix)
        self.cutmix_prob, self.cutmix_size, self.cutmix_ratio = float(cutmix_prob), tuple(cutmix_size), tuple(cutmix_ratio)
        if self.cutmix:
            from losses.weak_strong import WeakToStrongLoss
            self.w2s = WeakToStrongLoss(self.num_classes - 1, ce_weight=1.0, dice_weight=0.0)
        self.last_supervised = self.last_cps = self.last_agree = self.last_confident = None
        self.last_mask = self.last_perm = self.last_net_in = self.last_codes = None

    def _nets(self):
        return (self.model, self.model_b)

    def _steppers(self):
        return ((self.optimizer, self.lr_scheduler), (self.optimizer_b, self.lr_scheduler_b))

    def _dyn_values(self):
        return _ramp_value(self.cps_weight, self.current_iter), _ramp_value(self.confidence_threshold, self.current_iter)

    def _cutmix_loss(self, image: torch.Tensor, label: torch.Tensor) -> torch.Tensor:
        from losses.weak_strong import box_masks, random_cutmix_boxes
        lb = self.labeled_bs
        nu = image.shape[0] - lb
        self._write_dyn()
        image = image.contiguous()
        unlabeled = image[lb:]
        with torch.no_grad(), ops.no_bn_tracking():
            code_a, kept_a = ops.w2s_labels(self.model(unlabeled), self.dyn)
            code_b, kept_b = ops.w2s_labels(self.model_b(unlabeled), self.dyn)
        h, w = image.shape[2:]
        mask = box_masks(random_cutmix_boxes(nu, h, w, self.cutmix_prob, self.cutmix_size, self.cutmix_ratio), h, w, image.device)
        perm = torch.randperm(nu).to(torch.int32).to(image.device, non_blocking=True)
        net_in = torch.empty_like(image)
        net_in[:lb] = image[:lb]
        ops.cutmix_perm(unlabeled, perm, mask, out=net_in[lb:])
        out_a = self.model(net_in)
        out_b = self.model_b(net_in)
        sup = self.supervised_loss(out_a[:lb], label[:lb]) + self.supervised_loss(out_b[:lb], label[:lb])
        self.last_supervised = sup.detach()
        loss = sup + self.w2s(out_a[lb:], code_b, mask, perm, dyn=self.dyn)
        ce_a = self.w2s.last_ce
        loss = loss + self.w2s(out_b[lb:], code_a, mask, perm, dyn=self.dyn)
        self.last_cps = ce_a + self.w2s.last_ce
        self.last_agree, self.last_confident = None, torch.stack([kept_a, kept_b])
        self.last_mask, self.last_perm, self.last_net_in, self.last_codes = mask, perm, net_in, (code_a, code_b)
        return loss

    def _loss(self, image: torch.Tensor, label: torch.Tensor) -> torch.Tensor:
        lb = self.labeled_bs
        if self.cutmix and image.shape[0] > lb:
            return self._cutmix_loss(image, label)
        out_a = self.model(image)
        out_b = self.model_b(image)
        sup = self.supervised_loss(out_a[:lb], label[:lb]) + self.supervised_loss(out_b[:lb], label[:lb])
        self.last_supervised = sup.detach()
        s = 0 if self.cps_on_labeled else lb
        if image.shape[0] <= s:
            return sup
        self._write_dyn()
        loss = sup + self.cps(out_a[s:], out_b[s:], dyn=self.dyn)
        self.last_cps = self.cps.last_value_a + self.cps.last_value_b
        self.last_agree, self.last_confident = self.cps.last_agree, self.cps.last_confident
        return loss

    def _after_step(self) -> None:
        # B's step moved the parameter epoch on after A's packed weights were rebuilt; A's parameters have not changed since
        plan = self.optimizer._pack_plan
        if plan is not None and plan.valid():
            plan.plant()

    @torch.no_grad()
    def predict(self, image: torch.Tensor, use: str = "a") -> torch.Tensor:
        """eval forward -> arg-max of the soft-max of network "a", of network "b", or of the "mean" of the two soft-maxes
        (`inference.predictor.softmax_accum`: ties to the lowest class)."""
        if use not in ("a", "b", "mean"):
            raise ValueError(f'CPSEngine.predict: use="{use}" is none of "a", "b", "mean"')
        if use != "mean":
            return self._predict(self.model if use == "a" else self.model_b, image)
        image = image.to(self.optimizer.flat_param.device, dtype=torch.float32)
        from inference.predictor import softmax_accum
        self.model.eval()
        self.model_b.eval()
        za = self.model(image)
        prob = torch.empty(za.shape, device=za.device, dtype=torch.float32)
        pred = torch.empty((za.shape[0],) + tuple(za.shape[2:]), device=za.device, dtype=torch.int64)
        softmax_accum(za, prob, None, weight=0.5, first=True)
        softmax_accum(self.model_b(image), prob, pred, weight=0.5)
        return pred

    def save_state_dict(self, save_path, save_training_state: bool = False, **extra) -> None:
        """Network A as `TrainEngine.save_state_dict` writes it (model.pth, training_state.pth on request: the reference's layout);
        network B's `state_dict` -- and on request its optimizer state, in the same torch.optim format -- in a file of its own."""
        from training import checkpoint
        super().save_state_dict(save_path, save_training_state, **extra)
        peer = {"model": checkpoint.model_state_for_save(self.model_b)}
        if save_training_state:
            peer["optimizer"] = checkpoint.optimizer_state_to_torch(self.optimizer_b, self.model_b)
            peer["optimizer"]["step_count"] = int(self.optimizer_b.step_count)
        torch.save(peer, Path(save_path) / CPS_PEER_FILE)

    def load_state_dict(self, save_path) -> dict:
        from training import checkpoint
        out = super().load_state_dict(save_path)
        pf = Path(save_path) / CPS_PEER_FILE
        if pf.is_file():
            sd = torch.load(pf, map_location=self.optimizer_b.flat_param.device, weights_only=True)
            self.model_b.load_state_dict(sd["model"])  # copy_ into the flat-buffer views
            if "optimizer" in sd:
                checkpoint.optimizer_state_from_torch(self.optimizer_b, self.model_b, sd["optimizer"])
        ops.bump_param_epoch()  # packed weights of both networks are stale now
        return out


class VATEngine(SemiEngine):
    """one network + supervised loss on the labelled images + virtual adversarial training on the unlabelled ones + flat optimizer +
    poly LR.  `train_step` returns the loss TENSOR (no host sync); `last_supervised` and `last_vat` (unweighted) are device by-products
    of the latest step.  Per step, with lb = labeled_bs:

        z_clean = model(image[lb:])                         no gradient, batch-norm running statistics untouched
        x_adv   = vat.adversarial(model, image[lb:], z_clean, eps_dev=dyn[1:2])
        out     = model(cat([image[:lb], x_adv]))           ONE training forward, after the power pass has finished: `UNet.forward`
                                                            drops the producer -> consumer hints of the forward before it
        loss    = supervised_loss(out[:lb], label[:lb]) + vat(out[lb:], z_clean, dyn=dyn)

    With no unlabelled image or `vat=False` the engine forwards `image[:lb]` only and returns the supervised loss.
    vat: None = `VATLoss()`; a module with that interface; False = no adversarial term.
    vat_weight, eps: a float or an object with `.step(i)`; each step the engine writes `weight_i` and `eps_i` into the device buffer
    `dyn` before anything reads it, outside the autograd graph.  eps None = the `eps` of `vat`.
    The checkpoint is the base engine's: there is no extra state."""

    def __init__(self, model, supervised_loss, labeled_bs: int, vat=None, vat_weight=1.0, eps=None, optimizer_name: str = "adam",
                 optimizer_kwargs: Optional[dict] = None, start_lr: float = 1e-3, num_iters: int = 4000, lr_warmup_iter: int = 250,
                 lr_interval: int = 1, lr_scheduler_name: str = "poly", grad_norm: float = 10.0, process_group=None):
        super().__init__(model, labeled_bs, grad_norm, process_group, optimizer_name, optimizer_kwargs, start_lr, num_iters,
                         lr_warmup_iter, lr_interval, lr_scheduler_name)
        self.supervised_loss = supervised_loss
        if vat is None:
            from losses.vat_loss import VATLoss
            vat = VATLoss()
        self.vat = vat or None
        self.vat_weight = vat_weight
        self.eps = eps if eps is not None else (self.vat.eps if self.vat is not None else 0.0)
        self.last_supervised = self.last_vat = None

    def _dyn_values(self):
        return _ramp_value(self.vat_weight, self.current_iter), _ramp_value(self.eps, self.current_iter)

    def _loss(self, image: torch.Tensor, label: torch.Tensor) -> torch.Tensor:
        lb = self.labeled_bs
        if self.vat is None or image.shape[0] <= lb:
            sup = self.supervised_loss(self.model(image[:lb]), label[:lb])
            self.last_supervised = sup.detach()
            return sup
        self._write_dyn()
        unlabeled = image[lb:]
        with torch.no_grad(), ops.no_bn_tracking():
            z_clean = self.model(unlabeled)
        x_adv = self.vat.adversarial(self.model, unlabeled, z_clean, eps_dev=self.dyn[1:2])
        out = self.model(torch.cat([image[:lb], x_adv]))
        sup = self.supervised_loss(out[:lb], label[:lb])
        self.last_supervised = sup.detach()
        loss = sup + self.vat(out[lb:], z_clean, dyn=self.dyn)
        self.last_vat = getattr(self.vat, "last_value", None)
        return loss


class BCPEngine(_EMATeacher, SemiEngine):
    """student + EMA teacher + bidirectional copy-paste between labelled and unlabelled images + flat optimizer + poly LR.
    `train_step` returns the loss TENSOR (no host sync); `last_inward`, `last_outward` (the two loss terms) and `last_mask` (uint8
    [H, W]) are device by-products of the latest step.

    A batch is as for the siblings, with B = 2 * labeled_bs and labeled_bs even (anything else raises `ValueError`).  With h =
    labeled_bs / 2 the labelled halves are X_a, X_b with Y_a, Y_b and the unlabelled halves U_a, U_b.  A self-training step:

        z_t  = teacher([U_a; U_b])                  ONE pass, no gradient, train mode, no input noise (as published); BEFORE the
                                                    student's forward: `UNet.forward` clears the producer -> consumer hints
        P    = argmax z_t                           (`softmax_accum`); with `pseudo_largest_component` the largest connected component
                                                    of every foreground class and image is kept (`filter_components`)
        M    = random_box_mask(H, W, mask_ratio)    one mask for the batch; 1 outside the box
        in   = [M ? U_a : X_a ; M ? X_b : U_b]      two `ops.bcp_mix` calls into the halves of ONE network input: inward, outward
        out  = model(in)                            ONE student forward
        loss = CopyPasteLoss(out[:h], P_a, Y_a, M, u_weight, 1) + CopyPasteLoss(out[h:], Y_b, P_b, M, 1, u_weight)
        backward, clip, step; then the EMA with `ema_alpha(ema_step, ema_decay)`

    Where this departs from the published code: the mix is a selection, not `a * M + b * (1 - M)` (`ops.bcp_mix`); the two mixed
    batches go through the network in one forward where the published code runs two -- per image the same with instance norm, while
    with BATCH norm the statistics here span both mixes (two forwards of one network before a backward would also break the hint
    mechanism); the pseudo-labels are cleaned by true connected components per class, where the published code keeps the largest
    component of the foreground with a CPU library.  The Dice sums are per loss call (per mix), as published.

    `pretrain=True` is the published pre-training: only the labelled images are used, the input is `M ? X_a : X_b` (h rows), the
    loss `CopyPasteLoss(out, Y_a, Y_b, M, 1, 1)`, and the teacher is neither run nor updated.  `begin_self_training()` then makes the
    teacher the student bit for bit and clears `pretrain`.
    loss: None = `CopyPasteLoss` for the student's classes; a module with that call signature.
    Eager steps, one rank, 2-D inputs, index labels."""

    _one_rank_why = " (the EMA and the teacher pass are not sharded yet)"

    def __init__(self, model, teacher, labeled_bs: int, u_weight: float = 0.5, mask_ratio: float = 2 / 3, ema_decay: float = 0.99,
                 pseudo_largest_component: bool = True, pretrain: bool = False, loss=None, optimizer_name: str = "adam",
                 optimizer_kwargs: Optional[dict] = None, start_lr: float = 1e-3, num_iters: int = 4000, lr_warmup_iter: int = 250,
                 lr_interval: int = 1, lr_scheduler_name: str = "poly", grad_norm: float = 10.0, process_group=None):
        if not 0.0 <= ema_decay <= 1.0:
            raise ValueError("BCPEngine: ema_decay must lie in [0, 1]")
        if not 0.0 <= mask_ratio <= 1.0:
            raise ValueError("BCPEngine: mask_ratio must lie in [0, 1]")
        if labeled_bs < 2 or labeled_bs % 2:
            raise ValueError(f"BCPEngine: labeled_bs={labeled_bs} must be even and at least 2 (the labelled images are mixed in two halves)")
        super().__init__(model, labeled_bs, grad_norm, process_group, optimizer_name, optimizer_kwargs, start_lr, num_iters,
                         lr_warmup_iter, lr_interval, lr_scheduler_name)
        self.teacher = teacher
        self.ema_decay = float(ema_decay)
        self.u_weight, self.mask_ratio = float(u_weight), float(mask_ratio)
        self.pseudo_largest_component, self.pretrain = bool(pseudo_largest_component), bool(pretrain)
        self.num_classes = int(model.decoder.seg_output.weight.shape[0])  # K: background included
        if loss is None:
            from losses.copy_paste import CopyPasteLoss
            loss = CopyPasteLoss(self.num_classes - 1)
        self.loss = loss
        self._init_teacher()
        self.last_inward = self.last_outward = self.last_mask = None

    def _stage(self, sampled_batch):
        nimg, nlab = sampled_batch["image"].shape[0], sampled_batch["label"].shape[0]
        if nimg != 2 * self.labeled_bs or nlab < self.labeled_bs:
            raise ValueError(f"BCPEngine: {nimg} images / {nlab} label maps for labeled_bs={self.labeled_bs}; a batch holds labeled_bs "
                             f"labelled images followed by as many unlabelled ones")
        return super()._stage(sampled_batch)

    @torch.no_grad()
    def _pseudo_labels(self, unlabeled: torch.Tensor) -> torch.Tensor:
        """int64 [n, H, W]: the arg-max of ONE teacher pass, cleaned to the largest component per foreground class and image."""
        from inference.predictor import softmax_accum
        zt = self.teacher(unlabeled)
        pred = torch.empty((zt.shape[0],) + tuple(zt.shape[2:]), device=zt.device, dtype=torch.int64)
        softmax_accum(zt, None, pred, first=True)
        if self.pseudo_largest_component:
            from inference.components import filter_components
            pred = filter_components(pred, keep_largest=True, n_classes=self.num_classes)
        return pred

    def _mask(self, image: torch.Tensor) -> torch.Tensor:
        from losses.copy_paste import random_box_mask
        self.last_mask = random_box_mask(image.shape[2], image.shape[3], self.mask_ratio, device=image.device)
        return self.last_mask

    def _loss(self, image: torch.Tensor, label: torch.Tensor) -> torch.Tensor:
        lb = self.labeled_bs
        h = lb // 2
        xa, xb, ya, yb = image[:h], image[h:lb], label[:h], label[h:lb]
        if self.pretrain:
            mask = self._mask(image)
            loss = self.loss(self.model(ops.bcp_mix(xa, xb, mask)), ya, yb, mask, 1.0, 1.0)
            self.last_inward, self.last_outward = loss.detach(), None
            return loss
        pseudo = self._pseudo_labels(image[lb:])
        mask = self._mask(image)
        net_in = torch.empty((lb,) + tuple(image.shape[1:]), device=image.device, dtype=torch.float32)
        ops.bcp_mix(image[lb:lb + h], xa, mask, out=net_in[:h])  # inward: the labelled box inside an unlabelled image
        ops.bcp_mix(xb, image[lb + h:], mask, out=net_in[h:])    # outward: the unlabelled box inside a labelled image
        out = self.model(net_in)
        inward = self.loss(out[:h], pseudo[:h], ya, mask, self.u_weight, 1.0)
        outward = self.loss(out[h:], yb, pseudo[h:], mask, 1.0, self.u_weight)
        self.last_inward, self.last_outward = inward.detach(), outward.detach()
        return inward + outward

    def _after_step(self) -> None:
        if not self.pretrain:
            super()._after_step()

    def begin_self_training(self) -> None:
        """The end of pre-training: the teacher becomes the student bit for bit (parameters and buffers), `pretrain` is cleared."""
        with torch.no_grad():
            self.teacher.load_state_dict(self.model.state_dict())  # copy_ into the flat-buffer views, and the buffers
            self.teacher_flat.copy_(self.optimizer.flat_param)
        ops.bump_param_epoch()
        self.pretrain = False


class FixMatchEngine(SemiEngine):
    """one network + supervised loss on the labelled images + weak-to-strong consistency on the unlabelled ones + flat optimizer +
    poly LR.  `train_step` returns the loss TENSOR (no host sync).  Device by-products of the latest step: `last_supervised`;
    `last_unsup` (the unsupervised term as it enters the loss: the mean over the views of the WEIGHTED `WeakToStrongLoss`);
    `last_kept` (int64: confident pixels of the weak view); `last_code` (uint8 [nu, H, W], the weak view's code map); `last_masks`
    (per view uint8 [nu, H, W], 1 inside the CutMix box), `last_perms` (per view int32 [nu]) and `last_net_in` (the ONE input of the
    student's forward).  With lb = labeled_bs, U = image[lb:], nu = len(U), V = strong_views (1: FixMatch, 2: UniMatch's dual-stream
    perturbation), one step is

        zw = model(U)                               no gradient, batch-norm running statistics untouched (`ops.no_bn_tracking`);
                                                    BEFORE the student's forward: `UNet.forward` clears the producer -> consumer hints
        code, kept = ops.w2s_labels(zw, dyn)        arg-max and [confidence >= dyn[1]] per pixel, one byte
        for v in range(V):
            S_v    = strong_transform(U)            an intensity-only `BatchedAugment` (brightness, contrast, gamma, blur, noise; its
                                                    own draws per view); geometry untouched, so pixel p of S_v is pixel p of U;
                                                    None = identity
            mask_v = box_masks(random_cutmix_boxes(nu, H, W, cutmix_prob, cutmix_size, cutmix_ratio));  perm_v = torch.randperm(nu)
            net_in[lb + v nu : lb + (v + 1) nu] = ops.cutmix_perm(S_v, perm_v, mask_v)        straight into the rows of ONE input
        net_in[:lb] = image[:lb]
        out  = model(net_in)                        ONE student forward
        loss = supervised_loss(out[:lb], label[:lb]) + (1/V) sum_v w2s(out[rows of v], code, mask_v, perm_v, dyn=dyn)

    The images of the batch are the weak view: the geometric augmentation happens upstream in `BatchedAugment`, as for every engine
    here.  Boxes and permutations are drawn on the host (`torch.manual_seed` reproduces a run; nothing syncs).  With batch norm the
    statistics of the one forward span the labelled and the strong rows, as in the published code.  With no unlabelled image or
    `loss=False` the engine forwards `image[:lb]` only and returns the supervised loss.
    u_weight, confidence_threshold: a float or an object with `.step(i)`; each step the engine writes `weight_i` and `tau_i` into the
    device buffer `dyn` before anything reads it, outside the autograd graph.
    strong_transform: called as `strong_transform(U, zero labels)` -- a `BatchedAugment` with `inplace=False` and no resize, or any
    callable of that signature; the result is a dict with "image" or the image tensor itself, and must have U's shape.
    loss: None = `WeakToStrongLoss(K - 1, ce_weight, dice_weight)`; a module with that call signature; False = no unsupervised term.
    The checkpoint is the base engine's: there is no extra state.

    feature_perturbation=True adds UniMatch's third unlabelled stream (Yang et al., CVPR 2023): the decoder also runs on
    channel-dropped copies of the weak rows' encoder outputs (`UNet.forward(fp_rows=...)`, Dropout2d(fp_drop) on every skip tensor
    and the bottleneck), and the weak rows ride in the ONE student forward.  With N = lb + nu + V nu, one step is then

        net_in = [ image[:lb] ; U ; view_0 ; .. ; view_{V-1} ]          N rows, ONE input (`last_net_in`), ONE forward
        out    = model(net_in, fp_rows=(lb, nu), fp_drop=fp_drop)        [N + nu, K, H, W]
        zw     = out[lb : lb + nu].detach();   code, kept = ops.w2s_labels(zw, dyn)
        strong_v = w2s(out[lb + nu + v nu : lb + nu + (v + 1) nu], code, mask_v, perm_v, dyn=dyn)
        fp       = w2s(out[N : N + nu], code, dyn=dyn)                   no mix: pixel p of a perturbed row is pixel p of its weak row
        loss = supervised_loss(out[:lb], label[:lb]) + (1 - fp_weight) (1/V) sum_v strong_v + fp_weight fp

    V = 2 and fp_weight = 0.5 give the paper's 0.25 / 0.25 / 0.5 split of the unlabelled term.  The paper's overall (L_x + L_u) / 2
    is a scale of the learning rate and is not reproduced.  `last_fp` is the term as it enters the loss (fp_weight fp), `last_unsup`
    the whole unlabelled term; `loss` has the bits of `last_supervised + last_unsup`.  Differences from the flag-off step: there is no
    separate no-gradient weak pass -- the weak prediction is made inside the student's forward in train mode, so under batch norm it
    uses THIS batch's statistics (spanning labelled, weak, strong and, in the decoder, perturbed rows) instead of the weak batch's
    own, and it moves the running statistics; it is subject to the blocks' own dropout, as it already was.  The clean weak rows
    enter no loss term, so the decoder's backward carries zero gradients for them (their encoder work is what the new stream trains
    on).  The model must accept `fp_rows` / `fp_drop` (`models.unet.UNet`).  Eager steps, one rank, 2-D, like the rest of the engine."""

    def __init__(self, model, supervised_loss, labeled_bs: int, u_weight=1.0, confidence_threshold=0.95, strong_views: int = 1,
                 strong_transform=None, cutmix_prob: float = 0.5, cutmix_size=(0.02, 0.4), cutmix_ratio=(0.3, 1 / 0.3), loss=None,
                 ce_weight: float = 1.0, dice_weight: float = 0.0, optimizer_name: str = "adam",
                 optimizer_kwargs: Optional[dict] = None, start_lr: float = 1e-3, num_iters: int = 4000, lr_warmup_iter: int = 250,
                 lr_interval: int = 1, lr_scheduler_name: str = "poly", grad_norm: float = 10.0, process_group=None,
                 feature_perturbation: bool = False, fp_drop: float = 0.5, fp_weight: float = 0.5):
        if strong_views < 1:
            raise ValueError("FixMatchEngine: strong_views must be at least 1")
        if not 0.0 <= cutmix_prob <= 1.0:
            raise ValueError("FixMatchEngine: cutmix_prob must lie in [0, 1]")
        if not 0.0 <= fp_weight <= 1.0:
            raise ValueError("FixMatchEngine: fp_weight must lie in [0, 1]")
        if not 0.0 <= fp_drop < 1.0:
            raise ValueError("FixMatchEngine: fp_drop must lie in [0, 1)")
        if getattr(strong_transform, "inplace", False):
            raise ValueError("FixMatchEngine: strong_transform must not work in place (the unlabelled images are the weak view, and "
                             "every strong view starts from them)")
        super().__init__(model, labeled_bs, grad_norm, process_group, optimizer_name, optimizer_kwargs, start_lr, num_iters,
                         lr_warmup_iter, lr_interval, lr_scheduler_name)
        self.supervised_loss = supervised_loss
        self.u_weight, self.confidence_threshold = u_weight, confidence_threshold
        self.strong_views, self.strong_transform = int(strong_views), strong_transform
        self.cutmix_prob, self.cutmix_size, self.cutmix_ratio = float(cutmix_prob), tuple(cutmix_size), tuple(cutmix_ratio)
        self.num_classes = int(model.decoder.seg_output.weight.shape[0])  # K: background included
        if loss is None:
            from losses.weak_strong import WeakToStrongLoss
            loss = WeakToStrongLoss(self.num_classes - 1, ce_weight, dice_weight)
        self.w2s = loss or None
        self.feature_perturbation, self.fp_drop, self.fp_weight = bool(feature_perturbation), float(fp_drop), float(fp_weight)
        self.last_supervised = self.last_unsup = self.last_kept = self.last_code = self.last_fp = None
        self.last_masks = self.last_perms = self.last_net_in = None

    def _dyn_values(self):
        return _ramp_value(self.u_weight, self.current_iter), _ramp_value(self.confidence_threshold, self.current_iter)

    def _strong(self, unlabeled: torch.Tensor) -> torch.Tensor:
        if self.strong_transform is None:
            return unlabeled
        out = self.strong_transform(unlabeled, torch.zeros((unlabeled.shape[0],) + tuple(unlabeled.shape[2:]),
                                                           device=unlabeled.device, dtype=torch.int64))
        strong = out["image"] if isinstance(out, dict) else out
        if strong.shape != unlabeled.shape:
            raise ValueError(f"FixMatchEngine: strong_transform changed the shape {tuple(unlabeled.shape)} -> {tuple(strong.shape)}; "
                             f"the strong view must keep the geometry of the weak one")
        return strong.to(torch.float32).contiguous()

    def _loss(self, image: torch.Tensor, label: torch.Tensor) -> torch.Tensor:
        from losses.weak_strong import box_masks, random_cutmix_boxes
        lb = self.labeled_bs
        nu = image.shape[0] - lb
        if self.w2s is None or nu <= 0:
            sup = self.supervised_loss(self.model(image[:lb]), label[:lb])
            self.last_supervised = sup.detach()
            return sup
        self._write_dyn()
        image = image.contiguous()
        unlabeled = image[lb:]
        fp = self.feature_perturbation
        if not fp:
            with torch.no_grad(), ops.no_bn_tracking():
                zw = self.model(unlabeled)
            code, self.last_kept = ops.w2s_labels(zw, self.dyn)
        views = self.strong_views
        h, w = image.shape[2:]
        dev = image.device
        first = lb + nu if fp else lb  # the first strong row: with the feature-perturbation stream the weak rows ride in the forward
        rows = first + views * nu
        net_in = torch.empty((rows,) + tuple(image.shape[1:]), device=dev, dtype=torch.float32)
        masks, perms = [], []
        for v in range(views):
            strong = self._strong(unlabeled)
            mask = box_masks(random_cutmix_boxes(nu, h, w, self.cutmix_prob, self.cutmix_size, self.cutmix_ratio), h, w, dev)
            perm = torch.randperm(nu).to(torch.int32).to(dev, non_blocking=True)  # a permutation by construction: taken as it is
            ops.cutmix_perm(strong, perm, mask, out=net_in[first + v * nu:first + (v + 1) * nu])
            masks.append(mask)
            perms.append(perm)
        if fp:
            net_in[:first] = image
            out = self.model(net_in, fp_rows=(lb, nu), fp_drop=self.fp_drop)
            code, self.last_kept = ops.w2s_labels(out[lb:first].detach(), self.dyn)
        else:
            net_in[:lb] = image[:lb]
            out = self.model(net_in)
        sup = self.supervised_loss(out[:lb], label[:lb])
        self.last_supervised = sup.detach()
        unsup = None
        for v in range(views):
            term = self.w2s(out[first + v * nu:first + (v + 1) * nu], code, masks[v], perms[v], dyn=self.dyn)
            unsup = term if unsup is None else unsup + term
        if views > 1:
            unsup = unsup / views
        if fp:
            fp_term = self.fp_weight * self.w2s(out[rows:rows + nu], code, None, None, dyn=self.dyn)
            unsup = (1.0 - self.fp_weight) * unsup + fp_term
            self.last_fp = fp_term.detach()
        self.last_unsup, self.last_code = unsup.detach(), code
        self.last_masks, self.last_perms, self.last_net_in = masks, perms, net_in
        return sup + unsup


class DTCEngine(SemiEngine):
    """one network with a segmentation head and a level-set head + supervised loss on the labelled images + dual-task consistency on
    all of them + flat optimizer + poly LR.  `train_step` returns the loss TENSOR (no host sync); `last_supervised`,
    `last_consistency` and `last_sdf` (both unweighted) are device by-products of the latest step.  With lb = labeled_bs, one step is

        z, r = model(image, return_level_set=True)          ONE training forward of the whole batch; both heads are `ops.HeadFn` on
                                                            the last decoder activation
        loss = supervised_loss(z[:lb], label[:lb]) + dtc(z, r, label, lb, dyn=dyn)
             = supervised + dyn[0] * L_cons(all images) + dyn[1] * L_sdf(labelled images)

    where the loss computes `phi = signed_distance_map(label[:lb], K - 1)` and its extents on the device, every step, from the labels
    it is given (`losses/dual_task.py` is the definition).  A batch without unlabelled images still has both terms.
    model: a `models.unet.DualTaskUNet`; a plain `UNet` has no `decoder.ls_output` and is refused.
    dtc: None = `DualTaskConsistencyLoss(K - 1)`; a module with that call signature.  False is refused: without the term the
    level-set head is never trained, and a supervised engine says that better.
    consistency_weight, beta: a float or an object with `.step(i)`; each step the engine writes both into the device buffer `dyn`
    before anything reads it, outside the autograd graph.  The published values are a sigmoid ramp to 0.1 and 0.3.
    The checkpoint is the base engine's: the extra head is in the model's `state_dict`.  Eager steps, one rank, 2-D inputs."""

    def __init__(self, model, supervised_loss, labeled_bs: int, dtc=None, consistency_weight=0.1, beta=0.3,
                 optimizer_name: str = "adam", optimizer_kwargs: Optional[dict] = None, start_lr: float = 1e-3, num_iters: int = 4000,
                 lr_warmup_iter: int = 250, lr_interval: int = 1, lr_scheduler_name: str = "poly", grad_norm: float = 10.0,
                 process_group=None):
        if getattr(getattr(model, "decoder", None), "ls_output", None) is None:
            raise ValueError("DTCEngine needs a model with a level-set head (models.unet.DualTaskUNet): a plain UNet has no "
                             "decoder.ls_output, and the dual-task term compares the two heads")
        if dtc is False:
            raise ValueError("DTCEngine: dtc=False would train without the dual-task term and leave the level-set head untrained; "
                             "use a supervised engine for that")
        super().__init__(model, labeled_bs, grad_norm, process_group, optimizer_name, optimizer_kwargs, start_lr, num_iters,
                         lr_warmup_iter, lr_interval, lr_scheduler_name)
        self.supervised_loss = supervised_loss
        self.consistency_weight, self.beta = consistency_weight, beta
        self.num_classes = int(model.decoder.seg_output.weight.shape[0])  # K: background included
        if int(model.decoder.ls_output.weight.shape[0]) != self.num_classes - 1:
            raise ValueError(f"DTCEngine: the level-set head has {int(model.decoder.ls_output.weight.shape[0])} channels for "
                             f"{self.num_classes - 1} foreground classes")
        if dtc is None:
            from losses.dual_task import DualTaskConsistencyLoss
            dtc = DualTaskConsistencyLoss(self.num_classes - 1)
        self.dtc = dtc
        self.last_supervised = self.last_consistency = self.last_sdf = None

    def _dyn_values(self):
        return _ramp_value(self.consistency_weight, self.current_iter), _ramp_value(self.beta, self.current_iter)

    def _loss(self, image: torch.Tensor, label: torch.Tensor) -> torch.Tensor:
        lb = self.labeled_bs
        self._write_dyn()
        z, r = self.model(image, return_level_set=True)
        sup = self.supervised_loss(z[:lb], label[:lb])
        self.last_supervised = sup.detach()
        loss = sup + self.dtc(z, r, label, lb, dyn=self.dyn)
        self.last_consistency = getattr(self.dtc, "last_consistency", None)
        self.last_sdf = getattr(self.dtc, "last_sdf", None)
        return loss
