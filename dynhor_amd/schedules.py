"""Pure host-side schedules of the training loop (upstream Runner) and the data-parallel frame
assignment.  No device code here."""
import math

import torch


def lr_factor(iter_step: int, warm_up_end: int, end_iter: int, alpha: float) -> float:
    """Linear warm-up then cosine decay to alpha (upstream update_learning_rate)."""
    if iter_step < warm_up_end:
        return iter_step / warm_up_end
    progress = (iter_step - warm_up_end) / (end_iter - warm_up_end)
    return (math.cos(math.pi * progress) + 1.0) * 0.5 * (1 - alpha) + alpha


def cos_anneal_ratio(iter_step: int, anneal_end: float) -> float:
    """min(1, iter/anneal_end); 1 if anneal_end == 0 (upstream get_cos_anneal_ratio)."""
    if anneal_end == 0.0:
        return 1.0
    return min(1.0, iter_step / anneal_end)


def frame_slot(iter_step: int, rank: int, world: int) -> int:
    """Index into the shared frame permutation used by `rank` at `iter_step`: ranks take consecutive slots, so one
    iteration covers `world` distinct frames and the ranks never exchange rays (only the gradient)."""
    return iter_step * world + rank


def frame_names(n_images: int, stems=None):
    """The names frames go by in file names and selections: the dataset's stems, else 0000, 0001, ..."""
    return [str(s) for s in stems] if stems is not None else ["{:04d}".format(i) for i in range(n_images)]


def select_frames(spec, n_images: int, stems=None, what: str = "frames"):
    """Sorted frame indices of a selection: "none" / None / an empty list (no frame), "all", "every:K[:offset]" (the frames offset,
    offset + K, ...; 0 <= offset < K) or frame names (frame_names) as a list or a comma-separated string.  `what` names the setting
    in the errors."""
    if spec is None or (isinstance(spec, str) and spec == "none"):
        return []
    if isinstance(spec, str) and spec == "all":
        return list(range(n_images))
    if isinstance(spec, str) and spec.startswith("every:"):
        parts = spec.split(":")
        try:
            k = int(parts[1])
            off = int(parts[2]) if len(parts) > 2 else 0
        except (ValueError, IndexError):
            k, off = 0, 0
        if len(parts) > 3 or k < 1 or not 0 <= off < k:
            raise ValueError(f"{what}: 'every:K[:offset]' needs integers K >= 1 and 0 <= offset < K, got {spec!r}")
        return list(range(off, n_images, k))
    if isinstance(spec, str):
        items = [s.strip() for s in spec.split(",") if s.strip()]
    elif isinstance(spec, (list, tuple)):
        items = [str(s) for s in spec]
    else:
        raise ValueError(f"{what}: expected none, all, every:K[:offset] or frame names, got {spec!r}")
    index = {s: i for i, s in enumerate(frame_names(n_images, stems))}
    unknown = [s for s in items if s not in index]
    if unknown:
        raise ValueError(f"{what}: unknown frame(s) {unknown}; the dataset has {n_images} frames named like "
                         f"{frame_names(n_images, stems)[:3]}")
    return sorted({index[s] for s in items})


def split_holdout(spec, n_images: int, stems=None):
    """(training frames, held-out frames), both sorted, of the train.holdout setting `spec` (select_frames; "all" is refused).  A
    holdout that leaves no training frame raises."""
    if isinstance(spec, str) and spec == "all":
        raise ValueError("train.holdout: 'all' would leave no frame to train on")
    held = select_frames(spec, n_images, stems, "train.holdout")
    out = set(held)
    train = [i for i in range(n_images) if i not in out]
    if not train:
        raise ValueError(f"train.holdout: {spec!r} holds out all {n_images} frames and leaves none to train on")
    return train, held


class FramePermutation:
    """The shared frame permutation of the training loop (upstream image_perm, App. A.8): drawn from a seeded CPU
    generator that every rank owns a copy of, re-drawn once per epoch (= n_images slots).  Ranks take consecutive
    slots (frame_slot), so the e-th permutation is the same object on every rank whatever the world size.
    frames: the training frames when some are held out (train.holdout): the permutation then runs over len(frames) slots and its
    values are mapped through the list, so an epoch covers every training frame once and no other.  None: every frame, with exactly
    the draws and the state of a permutation that knows nothing of holdouts."""

    def __init__(self, n_images: int, seed: int, frames=None):
        self.frames = None if frames is None else [int(f) for f in frames]
        if self.frames is not None and (not self.frames or min(self.frames) < 0 or max(self.frames) >= int(n_images)):
            raise ValueError(f"FramePermutation: frames must be a non-empty list of indices in [0, {int(n_images)})")
        self.n = int(n_images) if self.frames is None else len(self.frames)
        self.gen = torch.Generator(device="cpu")
        self.gen.manual_seed(int(seed))
        self.perm = torch.randperm(self.n, generator=self.gen)
        self.epoch = 0

    def frame(self, slot: int) -> int:
        epoch = slot // self.n
        if epoch < self.epoch:
            raise ValueError("FramePermutation only moves forward (slot belongs to a past epoch)")
        while self.epoch < epoch:
            self.perm = torch.randperm(self.n, generator=self.gen)
            self.epoch += 1
        k = int(self.perm[slot % self.n])
        return k if self.frames is None else self.frames[k]

    def state_dict(self):
        return {"gen": self.gen.get_state(), "perm": self.perm.clone(), "epoch": self.epoch}

    def check_state(self, sd):
        """Raises when `sd` is the state of a permutation over another number of frames."""
        if int(sd["perm"].numel()) != self.n:
            raise ValueError(f"the checkpoint's frame permutation has {int(sd['perm'].numel())} entries but this run trains on "
                             f"{self.n} frames: train.holdout (or the dataset) differs from the run that wrote it")

    def load_state_dict(self, sd):
        self.check_state(sd)
        self.gen.set_state(sd["gen"].cpu())
        self.perm = sd["perm"].cpu().clone()
        self.epoch = int(sd["epoch"])
