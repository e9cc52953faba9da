"""Train on a dataset: the reference's epoch loop (trainer/trainer.py, trainer/trainer_swint_hsa_nsf.py, main.py) around
speinet_amd.trainer.Trainer, fed by speinet_amd.data.TrainLoader.

    python -m speinet_amd.fit --dir_data <train dir> --dir_data_test <validation dir> --save <experiment dir> [--model speinet|swint]
        [--batch_size 20 --patch_size 200 --lr 1e-4 --lr_decay 150 --gamma 0.5 --epochs 500 --print_every 100
         --n_frames_per_video 200 --no_augment --pre_train <ckpt> --resume --train_precision bf16x3|bf16 --residency device|host --seed 1]

Both directories hold blur/<clip>/*, gt/<clip>/* and (model speinet) label/<clip>.npy.  In place of `--dir_data`,

        --dir_sharp <dir of folders of sharp frames> [--blur_ratio 0.1 0.3 0.5 --blur_threshold 5 --no_replan --blur_light code|srgb|gamma:<g>
                                                      --blur_noise <shot>:<read> --blur_shake <len>|<lo>..<hi> --blur_frames runs|single
                                                      --blur_codec <q>|<lo>..<hi>]

trains from sharp high-frame-rate footage directly (an extension beyond the reference, which precomputes its sets): the frames stay on
the device as uint8, and every epoch e trains on the set `python -m speinet_amd.blurset --seed <seed + e>` would write under the same
recipe (the `--blur_*` options are blurset's `--light --noise --shake --frames --codec`; speinet_amd.recipe states them) — runs, labels,
references, noise levels, PSFs and JPEG qualities re-drawn, nothing written — and every batch is averaged, cropped and augmented by
one launch, with a codec by one more in place on the batch (data.SharpTrainLoader);
`--no_replan` keeps epoch 0's set.  The validation set stays a written one.  Names and defaults are those of the reference's
option/__init__.py and its SPEINet template.  Per epoch, in the reference's order: `scheduler.step()`, one `Trainer.step` per batch,
a log line every `print_every` batches, then `evaluate()` — eval mode, one full-size validation sample at a time through the model's
inference path in its configured `precision`, the reference's PSNR of the float output (spei_psnr_f32) — and the files of the
reference's experiment directory, so its tools keep working:

    <save>/model/model_latest.pt   state_dict in the reference layout (speinet_amd.checkpoint)
    <save>/model/model_best.pt     the same, when this epoch's PSNR is the best so far
    <save>/optimizer.pt            Adam's state_dict
    <save>/psnr_log.pt             one mean validation PSNR per finished epoch

`resume` loads model_latest.pt and optimizer.pt and steps the scheduler once per entry of psnr_log.pt (trainer/trainer.py:19-22); the
loader's sampler is advanced by as many epochs, so the resumed run continues with the epoch orders and draws an uninterrupted run
would see (torch's and numpy's generators — DropPath, the HEM masks — are re-seeded, not restored, as in the reference).
Multi-rank (one process per GPU under torch.distributed): `seed_rank`, and rank r takes every world-th batch of the shared epoch
order; rank 0 evaluates and writes the files.  That split is tested on the CPU (gloo); a multi-GPU run of this loop has not been made.
Not built: the logger's plots, forward_chop in training (the clip API has it: speinet_amd.tiles), save_images.  The data set itself and its labels come from speinet_amd.blurset and
speinet_amd.detector.
"""
from __future__ import annotations

import argparse
import os
import warnings
from typing import Optional

import torch

from . import checkpoint, ops
from .recipe import Recipe, add_arguments, from_args
from .trainer import Trainer, seed_rank


class Schedule:
    """StepLR(step_size=lr_decay, gamma) driven in the reference's order: `begin_epoch()` calls `scheduler.step()` BEFORE the epoch's
    batches (trainer_swint_hsa_nsf.py:18-24) and returns (epoch, lr).  Epoch numbers are `scheduler.last_epoch` — 1 for the first — and
    the rate drops at epoch lr_decay, one epoch earlier than with torch's documented order (optimizer first)."""

    def __init__(self, optimizer: torch.optim.Optimizer, lr_decay: int, gamma: float):
        self.optimizer = optimizer
        self.scheduler = torch.optim.lr_scheduler.StepLR(optimizer, step_size=lr_decay, gamma=gamma)

    def _step(self) -> None:
        with warnings.catch_warnings():
            # torch warns that lr_scheduler.step() came before optimizer.step(): that IS the reference's order, kept on purpose so that
            # every epoch trains at the learning rate the reference trains it at
            warnings.filterwarnings("ignore", message=r"Detected call of `lr_scheduler\.step\(\)` before `optimizer\.step\(\)`")
            self.scheduler.step()

    def begin_epoch(self):
        self._step()
        return self.scheduler.last_epoch, self.optimizer.param_groups[0]["lr"]

    def fast_forward(self, epochs: int) -> None:
        for _ in range(epochs):                              # trainer/trainer.py:21-22
            self._step()

    @property
    def epoch(self) -> int:
        return self.scheduler.last_epoch


def _swint_template() -> dict:
    from .synth import state_dict_template
    here = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    return state_dict_template(os.path.join(here, "tests", "golden", "state_dict_keys_swint.txt"))


def export(model: torch.nn.Module, path: str) -> None:
    """The module's state_dict in the reference layout: checkpoint.export for SPEINet (validated against its 1020-entry inventory); the
    swint model's is checked against its own key inventory."""
    from .speinet import SPEINet
    if isinstance(model, SPEINet):
        return checkpoint.export(model, path)
    sd = {k: v.detach().cpu().contiguous() for k, v in model.state_dict().items()}
    ref = _swint_template()
    bad = [k for k in ref if k not in sd and not k.endswith(checkpoint.DERIVED)] + [k for k in sd if k not in ref]
    if bad:
        raise RuntimeError(f"{path}: the module's state_dict differs from the swint key inventory in {len(bad)} entries; first: {bad[0]}")
    torch.save(sd, path)


def load_weights(model: torch.nn.Module, path: str) -> None:
    from .speinet import SPEINet
    if isinstance(model, SPEINet):
        checkpoint.load_into(model, path, strict=True)
    else:
        model.load_state_dict(checkpoint.read(path), strict=True)


class Fit:
    """The epoch loop.  `model` on its device, `loss` a speinet_amd.loss.Loss, `train_loader` a data.TrainLoader (or SharpTrainLoader,
    whose set is planned anew by every epoch: its plan is logged with the epoch's first batch); `val_set` a
    data.ClipSet(train=False) (or None: no evaluation, PSNR 0 is logged) with `val_store` its ClipStore (default: loaded here with the
    training store's residency)."""

    def __init__(self, model, loss, train_loader, val_set=None, val_store=None, save: str = ".", lr: float = 1e-4, lr_decay: int = 150,
                 gamma: float = 0.5, epochs: int = 500, print_every: int = 100, weight_decay: float = 0.0, resume: bool = False,
                 seed: int = 1, log=print):
        from .data import ClipStore
        self.model, self.loss, self.loader, self.val_set, self.save, self.epochs, self.print_every = model, loss, train_loader, val_set, save, epochs, print_every
        self.log = log if log is not None else (lambda *a: None)
        self.device = train_loader.device
        if float(train_loader.rgb_range) != 1.0 or float(getattr(model.cfg, "rgb_range", 1.0)) != 1.0:
            raise ValueError("Fit evaluates through the clip ingest kernel, which is built for rgb_range 1 (the reference's setting)")
        import torch.distributed as dist
        self.rank = dist.get_rank() if dist.is_available() and dist.is_initialized() else 0
        seed_rank(seed)
        sm = train_loader.sampler
        if sm.world > 1 and sm.n_batches() % sm.world:
            # the rank with the extra batch would wait in its gradient all-reduce for a peer that never comes
            raise ValueError(f"{sm.n_batches()} batches per epoch do not divide over {sm.world} ranks: choose a batch size that gives every "
                             "rank the same number of batches")
        self.trainer = Trainer(model, loss, lr=lr, weight_decay=weight_decay)
        self.schedule = Schedule(self.trainer.optimizer, lr_decay, gamma)
        self.psnr_log: list = []
        self.loss_log: list = []
        self._said_crop = False
        os.makedirs(os.path.join(save, "model"), exist_ok=True)
        if resume:
            load_weights(model, os.path.join(save, "model", "model_latest.pt"))
            self.trainer.optimizer.load_state_dict(torch.load(os.path.join(save, "optimizer.pt"), map_location=self.device, weights_only=True))
            self.psnr_log = [float(v) for v in torch.load(os.path.join(save, "psnr_log.pt"), weights_only=True).reshape(-1).tolist()]
            # optimizer.pt carries the rate of the epoch it was saved in.  The reference fast-forwards from THAT rate, so a run resumed
            # after the first decay trains at gamma times the scheduled rate from then on; here the fast-forward starts from the initial
            # rate, so the resumed run continues at the rate the schedule gives
            for group in self.trainer.optimizer.param_groups:
                group["lr"] = group.get("initial_lr", lr)
            self.schedule.fast_forward(len(self.psnr_log))
            for _ in range(len(self.psnr_log)):               # the finished epochs' orders and draws: the next epoch gets its own
                train_loader.sampler.epoch()
            self.log(f"Resumed after epoch {len(self.psnr_log)}")
        self.val_store = val_store
        if val_set is not None and val_store is None and self.rank == 0:
            self.val_store = ClipStore(val_set, residency=train_loader.store.residency, device=self.device, log=self.log)

    # ---- one epoch ------------------------------------------------------------------------------------------------
    def train_epoch(self) -> float:
        epoch, lr = self.schedule.begin_epoch()
        self.log("Epoch {:3d} with Lr {:.2e}".format(epoch, lr))
        total, n_batches = 0.0, 0
        terms_log = getattr(self.loss, "log", None)          # speinet_amd.loss.Loss: one list of per-term values per call
        mark = len(terms_log) if terms_log is not None else 0
        for batch, (inp, gt) in enumerate(self.loader):
            if batch == 0 and hasattr(self.loader.clipset, "summary"):
                self.log(self.loader.clipset.summary())      # a SharpClipSet: this epoch's runs
                for line in self.loader.clipset.noise_lines():   # ... and the noise levels drawn for its clips
                    self.log(line)
            total += self.trainer.step(inp, gt)
            n_batches += 1
            if (batch + 1) % self.print_every == 0:
                terms = ""
                if terms_log is not None and hasattr(self.loss, "terms") and len(terms_log) > mark:
                    # the epoch's running mean of every term, as the reference's display_loss (Loss/__init__.py:72-80)
                    seen = terms_log[mark:]
                    means = [sum(row[i] for row in seen) / len(seen) for i in range(len(self.loss.terms))]
                    terms = "".join("[{}: {:.4f}]".format(kind, v) for (_w, kind, _f), v in zip(self.loss.terms, means))
                # trainer_swint_hsa_nsf.py:43-49 (its `mid` term is a constant 0)
                self.log("[{}/{}]\tLoss : [total: {:.4f}]{}[mid: {:.4f}]".format((batch + 1) * self.loader.batch, len(self.loader.clipset), total / (batch + 1),
                                                                                terms, 0.0))
        mean = total / max(n_batches, 1)
        self.loss_log.append(mean)
        return mean

    def _frames(self, store, clip: int, frames, zero_at: Optional[int]) -> torch.Tensor:
        """uint8 frames of one clip -> fp32 [n,3,H20,W20], cropped at the bottom / right to multiples of 20 (what the model takes)."""
        u8 = store[clip][list(frames)].to(self.device, non_blocking=True)
        H, W = u8.shape[1:3]
        h, w = H - H % 20, W - W % 20
        if (h, w) != (H, W):
            if not self._said_crop:
                self.log(f"Validation frames are {W}x{H}: cropped at the bottom / right to {w}x{h} (multiples of 20)")
                self._said_crop = True
            u8 = u8[:, :h, :w].contiguous()
        x, _ = ops.frames_u8_in(u8)
        if zero_at is not None:
            x[zero_at].zero_()
        return x

    def evaluate(self) -> float:
        """Mean over the validation samples of the reference's PSNR (utils.calc_psnr: float output, shave 4), model.eval(), no grad."""
        vs, st = self.val_set, self.val_store
        self.model.eval()
        results = []
        with torch.no_grad(), torch.cuda.device(self.device):
            for idx in range(len(vs)):
                s = vs.sample(idx)
                frames = list(s.frames) + ([s.pre, s.sub] if vs.references else [])
                x = self._frames(st.blur, s.clip, frames, vs.n_seq if (vs.references and s.zero_pre) else None)
                gt = self._frames(st.gt, s.clip, [s.frames[vs.n_seq // 2]], None)
                out = self.model(x.unsqueeze(0))
                results.append(ops.psnr_f32(gt[0], out[0].contiguous(), shave=4, rgb_range=1.0))
            sums = torch.stack(results).cpu()                 # the one host sync of the pass
        values = [ops.psnr_of(float(a), float(b)) for a, b in sums.tolist()]
        return sum(values) / len(values)

    def save_files(self, is_best: bool) -> None:
        export(self.model, os.path.join(self.save, "model", "model_latest.pt"))
        if is_best:
            export(self.model, os.path.join(self.save, "model", "model_best.pt"))
        torch.save(self.trainer.optimizer.state_dict(), os.path.join(self.save, "optimizer.pt"))
        torch.save(torch.tensor(self.psnr_log, dtype=torch.float64), os.path.join(self.save, "psnr_log.pt"))

    def run(self) -> list:
        while self.schedule.epoch < self.epochs:              # trainer/trainer.py:43-44 terminate()
            mean = self.train_epoch()
            epoch = self.schedule.epoch
            if self.rank == 0:
                psnr = self.evaluate() if self.val_set is not None else 0.0
                self.psnr_log.append(psnr)
                best = int(torch.tensor(self.psnr_log, dtype=torch.float64).max(0)[1])     # trainer_swint_hsa_nsf.py:87 psnr_log.max(0)
                self.log("Epoch {:3d}: mean loss {:.4f}, average PSNR: {:.3f} (Best: {:.3f} @epoch {})".format(
                    epoch, mean, psnr, self.psnr_log[best], best + 1))
                self.save_files(is_best=(best + 1 == epoch))  # trainer_swint_hsa_nsf.py:94
            else:
                self.psnr_log.append(0.0)
        return self.psnr_log


def build_model(name: str, device, pre_train: Optional[str] = None, train_precision: str = "bf16x3", synthetic_seed: Optional[int] = None):
    from .speinet import default_args
    from .synth import synth_state_dict
    args = default_args()
    if name == "speinet":
        from .speinet import SPEINet
        net = SPEINet(args=args)
    elif name == "swint":
        from .swint import SPEINet
        net = SPEINet(n_sequence=3, args=args)
    else:
        raise ValueError(f"unknown model {name!r} (speinet, swint)")
    if synthetic_seed is not None:
        net.load_state_dict(synth_state_dict(net.state_dict(), seed=synthetic_seed), strict=True)
    if pre_train:
        load_weights(net, pre_train)
    net = net.to(device)
    net.train_precision = train_precision
    return net


def parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser(description="Train SPEINet (or its swint sub-model) on blur / gt / label folders, or on folders of sharp "
                                             "frames blurred per batch, on one MI355X")
    source = ap.add_mutually_exclusive_group(required=True)
    source.add_argument("--dir_data", help="a written training set: blur/<clip>/, gt/<clip>/ and label/<clip>.npy")
    source.add_argument("--dir_sharp", help="one folder of sharp high-frame-rate frames per clip; the blur is synthesised per batch")
    ap.add_argument("--blur_ratio", type=float, nargs="+", default=[0.5], help="--dir_sharp: share of sharp runs; several: one is drawn per clip")
    ap.add_argument("--blur_threshold", type=int, default=5, help="--dir_sharp: a run of at most this many frames is a sharp frame (label 1)")
    ap.add_argument("--no_replan", action="store_true", help="--dir_sharp: keep epoch 0's runs for every epoch")
    add_arguments(ap, "blur_", "--dir_sharp: ")                # --blur_light --blur_noise --blur_shake --blur_frames --blur_codec
    ap.add_argument("--dir_data_test", required=True)
    ap.add_argument("--save", required=True)
    ap.add_argument("--model", default="speinet", choices=("speinet", "swint"))
    ap.add_argument("--batch_size", type=int, default=20)
    ap.add_argument("--patch_size", type=int, default=200)
    ap.add_argument("--lr", type=float, default=1e-4)
    ap.add_argument("--lr_decay", type=int, default=150)
    ap.add_argument("--gamma", type=float, default=0.5)
    ap.add_argument("--epochs", type=int, default=500)
    ap.add_argument("--print_every", type=int, default=100)
    ap.add_argument("--n_frames_per_video", type=int, default=200)
    ap.add_argument("--no_augment", action="store_true")
    ap.add_argument("--loss", default="1*L1+2*HEM")
    ap.add_argument("--pre_train", default=None)
    ap.add_argument("--resume", action="store_true")
    ap.add_argument("--train_precision", default="bf16x3", choices=("f32", "bf16x3", "bf16"))
    ap.add_argument("--residency", default="device", choices=("device", "host"))
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--device", default="cuda:0")
    return ap


def main(argv=None) -> None:
    from .data import ClipSet, ClipStore, SharpClipSet, SharpStore, SharpTrainLoader, TrainLoader
    from .loss import Loss
    ap = parser()
    a = ap.parse_args(argv)
    given = [f for f, d in zip(Recipe._fields, Recipe()) if getattr(a, "blur_" + f) != d]
    if a.dir_data and given:
        ap.error(" ".join(f"--blur_{f} {getattr(a, 'blur_' + f)}" for f in given) + ": the recipe shapes the blur synthesised from --dir_sharp; a "
                 "written set (--dir_data) holds its blur already: make it with `python -m speinet_amd.blurset "
                 + " ".join(f"--{f}" for f in given) + "`")
    recipe = from_args(ap, a, "blur_")
    refs = a.model == "speinet"
    if a.dir_sharp and a.residency != "device":
        ap.error("--dir_sharp keeps the sharp frames on the device (--residency device); a set that does not fit is written with "
                 "`python -m speinet_amd.blurset` and trained with --dir_data")
    if a.dir_sharp:
        train_set = SharpClipSet(a.dir_sharp, a.blur_ratio, a.blur_threshold, seed=a.seed, n_frames_per_video=a.n_frames_per_video,
                                 references=refs, patch=a.patch_size, **recipe._asdict())
    else:
        train_set = ClipSet(a.dir_data, True, 3, a.n_frames_per_video, references=refs, patch=a.patch_size)
    val_set = ClipSet(a.dir_data_test, False, 3, a.n_frames_per_video, references=refs)
    net = build_model(a.model, a.device, a.pre_train, a.train_precision)
    if a.dir_sharp:
        store = SharpStore(train_set, device=a.device)
        loader = SharpTrainLoader(train_set, store, a.batch_size, a.patch_size, seed=a.seed, augment=not a.no_augment, replan=not a.no_replan)
    else:
        store = ClipStore(train_set, residency=a.residency, device=a.device)
        loader = TrainLoader(train_set, store, a.batch_size, a.patch_size, seed=a.seed, augment=not a.no_augment)
    Fit(net, Loss(a.loss, device=a.device), loader, val_set, save=a.save, lr=a.lr, lr_decay=a.lr_decay, gamma=a.gamma, epochs=a.epochs,
        print_every=a.print_every, resume=a.resume, seed=a.seed).run()


if __name__ == "__main__":
    main()
