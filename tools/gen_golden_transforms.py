"""Records ``tests/golden/transforms.npz`` from the reference's own ``PgTransform``, ``ProgressiveTransform``, ``transform_args`` and
``transform_batch_tv`` (data/progressive_callback.py) on the CPU, driven with a recording transform class.

    python tools/gen_golden_transforms.py     # needs the reference checkout (OTVAE_REFERENCE_ROOT), build container only

``oracle/ref_import.py`` replaces that module by an identity stand-in (the reference's VAE only needs its decorator); this tool, in its
own process, drops the stand-in and imports the real file, whose third-party imports (``torchvision.transforms.Compose``, Lightning's
``Callback`` / ``rank_zero_warn``) the stubs of ref_import satisfy.  ``PgCompose`` is not driven: the reference's ``__getitem__``
iterates a ``PgTransform``, which never ends.

Layout of the file (numbers and lists of names only):

    pg/keys               the varying keywords, in order                      pg/fixed_kernel_size   the fixed keyword
    pg/seq/<key>          the sequences handed in (unequal lengths)
    pg/noop [T]           1 where PgTransform[t] is NOOP, t = 0 .. num_steps + 2
    pg/<key> [T]          the value the transform class was built with at t (nan where NOOP)
    sched/schedule        the scheduled epochs                                 sched/epochs   the epochs walked
    sched/replaced [E]    1 where on_train_epoch_start replaced the method's transform
    sched/sigma [E]       the sigma of the transform in place after the epoch's hook (nan: still NOOP)
    sched/warned          number of warnings on a module without a decorated method
    args/batch            the three numbers of the batch handed to the decorated methods
    args/tv_out           what the method saw through transform_batch_tv() with a doubling transform
    args/plain_out        what the method saw through transform_args() (defaults) with the same transform
    args/noop_out         what the method saw through transform_batch_tv() before any transform was installed"""
import importlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import ref_import as R  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "transforms.npz")
SEQ = {"sigma": [3.0, 2.0, 1.0, 0.5], "gain": [10.0, 20.0]}
SCHEDULE, EPOCHS = [0, 2, 3], list(range(7))


class Rec:
    """the recording transform: keeps the keywords it was built with, doubles what it is called on"""

    def __init__(self, **kwargs):
        self.kwargs = kwargs

    def __call__(self, x):
        return 2 * x


class Trainer:
    current_epoch = 0


def main():
    R.install()
    del sys.modules["ot_vae_lightning.data.progressive_callback"]     # ref_import's identity stand-in
    P = importlib.import_module("ot_vae_lightning.data.progressive_callback")
    warned = []
    P.rank_zero_warn = lambda *a, **k: warned.append(a)
    out = {}

    pg = P.PgTransform(Rec, SEQ, kernel_size=5)
    steps = list(range(pg.num_steps + 3))
    built = [pg[t] for t in steps]
    out["pg/keys"] = np.array(list(SEQ))
    out["pg/fixed_kernel_size"] = np.array(5)
    out["pg/num_steps"] = np.array(pg.num_steps)
    for k, seq in SEQ.items():
        out[f"pg/seq/{k}"] = np.array(seq)
        out[f"pg/{k}"] = np.array([np.nan if isinstance(b, P.NOOP) else b.kwargs[k] for b in built])
    out["pg/noop"] = np.array([int(isinstance(b, P.NOOP)) for b in built])
    assert all(isinstance(b, P.NOOP) or b.kwargs["kernel_size"] == 5 for b in built)

    class Module:
        seen = None

        @P.transform_batch_tv()
        def batch_preprocess(self, batch):
            self.seen = batch
            return batch

        @P.transform_args()
        def plain(self, x):
            self.seen = x
            return x

        def undecorated(self, x):
            return x

    class Bare:
        def method(self, x):
            return x

    m, trainer = Module(), Trainer()
    batch = (1.5, 7.0, -2.0)
    m.batch_preprocess(batch)
    out["args/batch"] = np.array(batch)
    out["args/noop_out"] = np.array(m.seen)

    cb = P.ProgressiveTransform(P.PgTransform(Rec, {"sigma": [1.0, 0.5]}, kernel_size=5), schedule=SCHEDULE)
    replaced, sigma = [], []
    for e in EPOCHS:
        trainer.current_epoch = e
        before = Module.batch_preprocess.__wrapped__.transform
        cb.on_train_epoch_start(trainer, m)
        after = Module.batch_preprocess.__wrapped__.transform
        replaced.append(int(after is not before))
        sigma.append(after.kwargs["sigma"] if isinstance(after, Rec) else np.nan)
        if e == 0:
            m.batch_preprocess(batch)
            out["args/tv_out"] = np.array(m.seen)
            m.plain(batch[0])
            out["args/plain_out"] = np.array(m.seen)
    out["sched/schedule"], out["sched/epochs"] = np.array(SCHEDULE), np.array(EPOCHS)
    out["sched/replaced"], out["sched/sigma"] = np.array(replaced), np.array(sigma)
    assert not warned
    trainer.current_epoch = 0
    cb.on_train_epoch_start(trainer, Bare())
    out["sched/warned"] = np.array(len(warned))

    np.savez_compressed(OUT, **out)
    for k, v in out.items():
        print(k, v.tolist())


if __name__ == "__main__":
    main()
