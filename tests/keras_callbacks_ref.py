"""The three Keras callbacks of a fit, restated from SURVEY.md A.5 as three separate objects, and the scripted val_loss
sequences the callback tests run (tests/test_references.py on the CPU, tests/test_gpu_callbacks.py on the device).

Written from the survey text alone: it imports neither locator_amd.train.Callbacks nor oracle.Callbacks, which are the
implementations it is compared with.  All three callbacks watch val_loss in mode "min" with min_delta 0; every comparison
is np.less, so a NaN never improves and +inf never improves on the initial +inf."""
import numpy as np


class ModelCheckpoint:
    """save_best_only: best = +inf; `if val_loss < best: best = val_loss; save`.  Ties do not save."""

    def __init__(self):
        self.best = np.inf

    def on_epoch_end(self, epoch, val_loss):
        if np.less(val_loss, self.best):
            self.best = val_loss
            return True
        return False


class EarlyStopping:
    """min_delta 0, patience P: `wait += 1; if val_loss < best: best = val_loss; wait = 0`, then
    `if wait >= P and epoch > 0: stop`."""

    def __init__(self, patience):
        self.patience = int(patience)
        self.best = np.inf
        self.wait = 0

    def on_epoch_end(self, epoch, val_loss):
        self.wait += 1
        if np.less(val_loss, self.best):
            self.best = val_loss
            self.wait = 0
        return bool(self.wait >= self.patience and epoch > 0)


class ReduceLROnPlateau:
    """cooldown 0, min_lr 0: logs the current LR first, then `if val_loss < best: best = val_loss; wait = 0` else
    `wait += 1; if wait >= patience: lr <- max(lr * factor, 0); wait = 0`.  The LR lives in an fp32 variable; Keras
    forms the product in double and rounds on assignment, which for a power-of-two factor is the fp32 product."""

    def __init__(self, lr_patience, factor, lr0):
        self.patience = int(lr_patience)
        self.factor = float(factor)
        self.lr = np.float32(lr0)
        self.best = np.inf
        self.wait = 0

    def on_epoch_end(self, epoch, val_loss):
        """-> (LR the epoch trained with, reduced?)"""
        logged = self.lr
        reduced = False
        if np.less(val_loss, self.best):
            self.best = val_loss
            self.wait = 0
        else:
            self.wait += 1
            if self.wait >= self.patience:
                self.lr = np.float32(max(float(self.lr) * self.factor, 0.0))
                self.wait = 0
                reduced = True
        return logged, reduced


class KerasCallbacks:
    """The callback list of locator.py:362 in its order: checkpoint -> early stopping -> LR plateau."""

    def __init__(self, patience, lr_patience, factor, lr0):
        self.ck = ModelCheckpoint()
        self.es = EarlyStopping(patience)
        self.rl = ReduceLROnPlateau(lr_patience, factor, lr0)

    def on_epoch_end(self, epoch, val_loss):
        """-> (save, stop, lr_logged, reduced)"""
        save = self.ck.on_epoch_end(epoch, val_loss)
        stop = self.es.on_epoch_end(epoch, val_loss)
        logged, reduced = self.rl.on_epoch_end(epoch, val_loss)
        return save, stop, logged, reduced


def device_trace(vals, patience, lr_patience, factor, lr0):
    """What the device's state has to be after every epoch of the val_loss sequence `vals`: the Keras callbacks above, plus
    what include/locator_hip.h adds for epochs enqueued behind the stop epoch - only `epoch` advances, save_now is 0, no
    history row.  -> one dict per epoch: the loc_cb_state fields, `lr_mirror`, and `row` = (val_loss, lr_logged, flags) or
    None where no history row may be written."""
    cb = KerasCallbacks(patience, lr_patience, factor, lr0)
    stopped, stop_epoch, best_epoch = 0, -1, -1
    out = []
    for epoch, v in enumerate(vals):
        v = np.float64(v)
        save, row = False, None
        if not stopped:
            save, stop, logged, reduced = cb.on_epoch_end(epoch, v)
            if save:
                best_epoch = epoch
            if stop:
                stopped, stop_epoch = 1, epoch
            row = (v, np.float64(logged), float(1 * save + 2 * stop + 4 * reduced))
        out.append({"ck_best": cb.ck.best, "es_best": cb.es.best, "rl_best": cb.rl.best, "es_wait": cb.es.wait,
                    "rl_wait": cb.rl.wait, "lr": cb.rl.lr, "lr_mirror": cb.rl.lr, "epoch": epoch + 1, "stopped": stopped,
                    "stop_epoch": stop_epoch, "best_epoch": best_epoch, "save_now": int(save), "row": row})
    return out


# ---------------------------------------------------------------- scripted val_loss sequences
# Every value is exact in fp32 (the device sees validation distances that are all this value, so their mean is the value
# itself and ties are real ties).
NAN, INF = float("nan"), float("inf")

MAIN = (
    [3.0, 2.75, 2.5, 2.25, 2.0, 1.75, 1.5, 1.375, 1.25, 1.0]      # 0-9   steady improvement
    + [1.0]                                                         # 10    an exact tie with the best: no save, waits 1
    + [0.875]                                                       # 11    improvement: both waits back to 0
    + [0.9375, 0.875, 1.5, 0.890625]                                # 12-15 plateau (a tie inside): two LR reductions at lr_patience 2
    + [0.75, 0.625]                                                 # 16-17 improvement resets both waits
    + [0.625, 0.75, 0.6875, 0.625, 2.0, 0.65625, 0.625, 0.625,      # 18-33 final plateau: early stopping fires at patience 5, 6
       0.75, 0.875, 0.625, 0.640625, 0.625, 0.75, 0.625, 0.625]     #       and 12, and at least three epochs follow the stop
)
assert len(MAIN) == 34 and all(float(np.float32(v)) == v for v in MAIN)

# name -> (val_loss sequence, patience, lr_patience, factor); lr0 is 1e-3 everywhere
SEQUENCES = {}
for _p, _lp in ((6, 1), (12, 2), (5, 0)):
    for _f in (0.5, 0.25):
        SEQUENCES[f"main-p{_p}-lp{_lp}-f{_f}"] = (MAIN, _p, _lp, _f)
SEQUENCES.update({
    # patience 1 and 0: early stopping can fire at epoch 1 and never at epoch 0, even where wait >= patience there
    "patience1-nan-first": ([NAN, 1.0, 1.0, 0.5, 0.5], 1, 0, 0.5),
    "patience1-flat": ([1.0, 1.0, 1.0, 1.0, 1.0], 1, 0, 0.5),
    "patience1-improving": ([2.0, 1.0, 1.5, 0.5, 0.25], 1, 0, 0.5),
    "patience0-flat": ([1.0, 1.0, 1.0, 1.0, 1.0], 0, 0, 0.5),
    "patience0-improving": ([2.0, 1.0, 0.5, 0.25, 0.125], 0, 0, 0.5),
    # NaN never improves: best_epoch stays -1, nothing is ever saved
    "nan-first-never-better": ([NAN, NAN, INF, NAN, INF, NAN, NAN, NAN, NAN, NAN], 6, 1, 0.5),
    "nan-first-then-finite": ([NAN, 2.0, 1.0, NAN, 1.0, 0.5, NAN, NAN, NAN, NAN, NAN, NAN, NAN, NAN, NAN], 6, 1, 0.5),
    "nan-in-the-middle": ([2.0, 1.5, NAN, 1.25, NAN, NAN, 1.0, INF, NAN, 1.0, 1.0, NAN, 1.0, 1.0, 1.0, 1.0], 6, 1, 0.25),
    "inf-first": ([INF, INF, 3.0, INF, 2.0, 2.0, INF, 2.5, INF, INF, INF, INF, INF, INF], 6, 1, 0.5),
})
LR0 = 1e-3
