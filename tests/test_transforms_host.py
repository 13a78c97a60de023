"""CPU: the host logic of ``ot_vae_lightning_amd.transforms`` and ``utils.Collage`` -- the progressive-transform rules against
tests/golden/transforms.npz (recorded from the reference's data/progressive_callback.py by tools/gen_golden_transforms.py with a
recording transform class), ``PgCompose``, the PNG writer and the routing of ``Collage.log_images``.  No kernel runs here."""
import struct
import types
import warnings
import zlib

import numpy as np
import pytest
import torch

from conftest import load_golden


@pytest.fixture(scope="module")
def gold():
    return load_golden("transforms.npz")


@pytest.fixture(scope="module")
def T():
    from ot_vae_lightning_amd import transforms
    return transforms


class Rec:
    """as the recorder of tools/gen_golden_transforms.py: keeps its keywords, doubles its argument"""

    def __init__(self, **kwargs):
        self.kwargs = kwargs

    def __call__(self, x):
        return 2 * x


def _module(T):
    class Module:
        seen = None

        @T.transform_batch_tv()
        def batch_preprocess(self, batch):
            self.seen = batch
            return batch

        @T.transform_args()
        def plain(self, x):
            self.seen = x
            return x

        def undecorated(self, x):
            return x

    return Module


def test_pg_transform_indexing_matches_the_reference(T, gold):
    keys = [str(k) for k in gold["pg/keys"]]
    seq = {k: gold[f"pg/seq/{k}"].tolist() for k in keys}
    assert len({len(v) for v in seq.values()}) > 1, "the golden must hold sequences of unequal length"
    pg = T.PgTransform(Rec, seq, kernel_size=int(gold["pg/fixed_kernel_size"]))
    assert pg.num_steps == int(gold["pg/num_steps"])
    noop = gold["pg/noop"]
    assert len(noop) == pg.num_steps + 3
    for t, is_noop in enumerate(noop):
        built = pg[t]
        assert isinstance(built, T.NOOP) == bool(is_noop), t
        if not is_noop:
            assert built.kwargs["kernel_size"] == int(gold["pg/fixed_kernel_size"])
            for k in keys:
                assert built.kwargs[k] == float(gold[f"pg/{k}"][t]), (t, k)
    obj = object()
    assert T.NOOP()(obj) is obj


def test_progressive_transform_schedule_matches_the_reference(T, gold):
    Module = _module(T)
    m, other = Module(), Module()
    trainer = types.SimpleNamespace(current_epoch=0)
    cb = T.ProgressiveTransform(T.PgTransform(Rec, {"sigma": [1.0, 0.5]}, kernel_size=5), schedule=gold["sched/schedule"].tolist())
    batch = tuple(gold["args/batch"].tolist())

    def active(mod):
        return mod.__dict__.get("_otvae_active_transforms", {}).get("batch_preprocess", Module.batch_preprocess.__wrapped__.transform)

    m.batch_preprocess(batch)
    assert m.seen == tuple(gold["args/noop_out"].tolist())
    for e, replaced, sigma in zip(gold["sched/epochs"].tolist(), gold["sched/replaced"].tolist(), gold["sched/sigma"].tolist()):
        trainer.current_epoch = e
        before = active(m)
        with warnings.catch_warnings():
            warnings.simplefilter("error")        # a decorated method exists: no warning
            cb.on_train_epoch_start(trainer, m)
        after = active(m)
        assert (after is not before) == bool(replaced), e
        assert (after.kwargs["sigma"] == sigma) if isinstance(after, Rec) else np.isnan(sigma), e
        if e == 0:
            m.batch_preprocess(batch)
            assert m.seen == tuple(gold["args/tv_out"].tolist())
            m.plain(batch[0])
            assert m.seen == float(gold["args/plain_out"])
    # the deliberate difference: the transform lives on the instance, a second module (and the class) keep NOOP
    assert isinstance(Module.batch_preprocess.__wrapped__.transform, T.NOOP)
    other.batch_preprocess(batch)
    assert other.seen == batch and "_otvae_active_transforms" not in other.__dict__


def test_progressive_transform_warns_without_a_decorated_method(T, gold):
    class Bare:
        def method(self, x):
            return x

    cb = T.ProgressiveTransform(T.PgTransform(Rec, {"sigma": [1.0]}), schedule=[0])
    with pytest.warns(UserWarning, match="didn't find any method") as rec:
        cb.on_train_epoch_start(types.SimpleNamespace(current_epoch=0), Bare())
    assert len(rec) == int(gold["sched/warned"]) == 1
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        cb.on_train_epoch_start(types.SimpleNamespace(current_epoch=1), Bare())   # not a scheduled epoch: nothing happens


def test_pg_compose_takes_step_t_of_every_member_and_terminates(T):
    a = T.PgTransform(Rec, {"sigma": [3.0, 2.0, 1.0]}, tag="a")
    b = T.PgTransform(Rec, {"gain": [10.0]}, tag="b")
    pc = T.PgCompose([a, b])
    for t, (sigma, b_noop) in enumerate([(3.0, False), (2.0, False), (1.0, True), (1.0, True)]):
        comp = pc[t]
        assert isinstance(comp, T.Compose) and len(comp.transforms) == 2
        assert comp.transforms[0].kwargs == {"sigma": sigma, "tag": "a"}
        assert isinstance(comp.transforms[1], T.NOOP) == b_noop
        assert comp(1.0) == (2.0 if b_noop else 4.0)
    assert all(isinstance(x, T.NOOP) for x in pc[4].transforms)
    assert T.PgCompose([a], compose_cls=list)[0][0].kwargs["sigma"] == 3.0


def test_gaussian_blur_constructor_keeps_torchvisions_checks(T):
    g = T.GaussianBlur(5, sigma=(1.5, 1.5))
    assert isinstance(g, torch.nn.Module) and g.kernel_size == (5, 5) and g.sigma == (1.5, 1.5)
    assert T.GaussianBlur((3, 7), 2).sigma == (2.0, 2.0) and T.GaussianBlur(3).sigma == (0.1, 2.0)
    for bad in (4, 0, -3, (3, 4), (3, 3, 3)):
        with pytest.raises(ValueError):
            T.GaussianBlur(bad)
    for bad in (0, -1.0, (0.0, 1.0), (2.0, 1.0), (1.0, 2.0, 3.0), "x"):
        with pytest.raises(ValueError):
            T.GaussianBlur(5, sigma=bad)
    torch.manual_seed(11)
    want = torch.empty(1).uniform_(0.5, 2.0).item()
    torch.manual_seed(11)
    assert T.GaussianBlur.get_params(0.5, 2.0) == want
    with pytest.raises(RuntimeError):      # no CPU path
        g(torch.zeros(1, 1, 8, 8))


def _read_png(path):
    blob = open(path, "rb").read()
    assert blob[:8] == b"\x89PNG\r\n\x1a\n"
    pos, chunks = 8, []
    while pos < len(blob):
        (n,), tag = struct.unpack(">I", blob[pos:pos + 4]), blob[pos + 4:pos + 8]
        data = blob[pos + 8:pos + 8 + n]
        (crc,) = struct.unpack(">I", blob[pos + 8 + n:pos + 12 + n])
        assert crc == zlib.crc32(tag + data) & 0xFFFFFFFF
        chunks.append((tag, data))
        pos += 12 + n
    assert [t for t, _ in chunks][0] == b"IHDR" and chunks[-1] == (b"IEND", b"")
    w, h, depth, colour, comp, filt, interlace = struct.unpack(">IIBBBBB", chunks[0][1])
    assert (depth, colour, comp, filt, interlace) == (8, 2, 0, 0, 0)
    raw = np.frombuffer(zlib.decompress(b"".join(d for t, d in chunks if t == b"IDAT")), np.uint8).reshape(h, 1 + 3 * w)
    assert (raw[:, 0] == 0).all(), "filter type 0 on every scanline"
    return raw[:, 1:].reshape(h, w, 3)


def test_png_writer_round_trips(tmp_path):
    from ot_vae_lightning_amd.utils.collage import write_png
    img = np.random.default_rng(0).integers(0, 256, (7, 5, 3), dtype=np.uint8)
    write_png(str(tmp_path / "a.png"), img)
    assert np.array_equal(_read_png(str(tmp_path / "a.png")), img)
    write_png(str(tmp_path / "b.png"), torch.from_numpy(img))
    assert np.array_equal(_read_png(str(tmp_path / "b.png")), img)
    with pytest.raises(ValueError):
        write_png(str(tmp_path / "c.png"), img[:, :, :1])


def _cpu_collage(images, num_samples, as_uint8=False):
    """``functional.collage`` on the host, for the routing test (n > 1 only)"""
    x = torch.cat(list(images), -1).clamp(0, 1)[:num_samples]
    n, c, h, w = x.shape
    x = x.expand(n, 3, h, w) if c == 1 else x
    grid = torch.zeros(3, n * (h + 2) + 2, w + 4)
    for k in range(n):
        grid[:, k * (h + 2) + 2:k * (h + 2) + 2 + h, 2:2 + w] = x[k]
    return grid.mul(255).add(0.5).clamp(0, 255).permute(1, 2, 0).to(torch.uint8) if as_uint8 else grid


class _Model:
    def batch_preprocess(self, batch):
        return {"samples": batch[0]}

    def not_marked(self, batch):
        raise AssertionError("only decorated methods are called")



def test_collage_log_images_routes_to_loggers_and_files(monkeypatch, tmp_path):
    import ot_vae_lightning_amd as A
    from ot_vae_lightning_amd import functional as HF
    monkeypatch.setattr(HF, "collage", _cpu_collage)
    monkeypatch.chdir(tmp_path)

    class Model(_Model):
        @A.Collage.log_method
        def pictures(self, batch):
            return [batch["samples"], 1 - batch["samples"]]

        @A.Collage.log_method
        def empty(self, batch):
            return []

    x = torch.rand(4, 1, 3, 5) * 2 - 0.5
    want = _cpu_collage([x, 1 - x], 3)
    cb, model = A.Collage(num_samples=3), Model()

    calls = []
    wandb_like = types.SimpleNamespace(log_image=lambda key, images, step=None: calls.append((key, images, step)))
    cb.on_validation_batch_end(types.SimpleNamespace(logger=wandb_like, global_step=7, is_global_zero=True), model, None, (x, None), 0)
    (key, images, step), = calls
    assert key == "val/collage/pictures" and step == 7 and len(images) == 1 and torch.equal(images[0], want)
    cb.on_validation_batch_end(types.SimpleNamespace(logger=wandb_like, global_step=8, is_global_zero=True), model, None, (x, None), 1)
    assert len(calls) == 1, "only the first batch is logged"

    calls.clear()
    tb_like = types.SimpleNamespace(experiment=types.SimpleNamespace(
        add_image=lambda key, image, global_step=None: calls.append((key, image, global_step))))
    cb.on_test_batch_end(types.SimpleNamespace(logger=tb_like, global_step=9, is_global_zero=True), model, None, (x, None), 0)
    (key, image, step), = calls
    assert key == "test/collage/pictures" and step == 9 and torch.equal(image, want)

    with pytest.warns(UserWarning, match="No logger found"):
        cb.log_images(types.SimpleNamespace(logger=None, global_step=12), model, (x, None))
    assert np.array_equal(_read_png(str(tmp_path / "collages" / "0012_pictures.png")), _cpu_collage([x, 1 - x], 3, True).numpy())

    with pytest.raises(NotImplementedError):
        cb.log_images(types.SimpleNamespace(logger=object(), global_step=0), model, (x, None))
    with pytest.warns(UserWarning, match="didn't find any method"):
        cb.log_images(types.SimpleNamespace(logger=wandb_like, global_step=0), _Model(), (x, None))


def test_list_to_collage_of_nothing_is_none_and_models_are_marked():
    import ot_vae_lightning_amd as A
    assert A.Collage.list_to_collage([], 8) is None
    assert A.AutoDiffusion.reconstruction.is_collage is True
    assert A.AutoDiffusion.generation.is_collage and A.AutoDiffusion.generation_improved.is_collage
    assert A.VAE.reconstruction.is_collage and A.VAE.generation.is_collage
    assert not hasattr(A.VAE.forward, "is_collage")
    assert A.utils.Collage is A.Collage and A.transforms.GaussianBlur is A.GaussianBlur
    assert isinstance(A.VAE.batch_preprocess.__wrapped__.transform, A.NOOP)
    with pytest.raises(RuntimeError):      # no CPU path
        A.Collage.list_to_collage([torch.zeros(2, 1, 4, 4)], 2)


def test_functional_argument_checks_come_before_any_kernel():
    from ot_vae_lightning_amd import functional as HF
    x = torch.zeros(1, 1, 8, 8)
    for k in (4, 0, -1, (3, 2), 2.0):
        with pytest.raises(ValueError, match="odd and positive"):
            HF.gaussian_blur(x, k, 1.0)
    for s in (0.0, -1.0, (1.0, 0.0)):
        with pytest.raises(ValueError, match="sigma should have positive values"):
            HF.gaussian_blur(x, 3, s)
    with pytest.raises((RuntimeError, NotImplementedError)):
        HF.gaussian_blur(x, 3, 1.0)
    from torch._subclasses.fake_tensor import FakeTensorMode
    for name in ("gaussian_blur", "gaussian_blur_backward"):
        assert torch._C._dispatch_has_kernel_for_dispatch_key(f"otvae::{name}", "CUDA")
        assert not torch._C._dispatch_has_kernel_for_dispatch_key(f"otvae::{name}", "CPU")
    with FakeTensorMode():
        a = torch.empty(2, 3, 9, 9, device="cuda")
        b = torch.empty(2, 9, 9, 3, device="cuda").permute(0, 3, 1, 2)
        assert torch.ops.otvae.gaussian_blur(a, 5, 5, 1.0, 1.0).stride() == a.stride()
        assert torch.ops.otvae.gaussian_blur(b, 5, 3, 1.0, 2.0).stride() == b.stride()
        assert torch.ops.otvae.gaussian_blur(a[0], 5, 5, 1.0, 1.0).shape == (3, 9, 9)
