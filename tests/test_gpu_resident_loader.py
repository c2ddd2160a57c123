"""GPU: the device-resident loader - tl_gather_rows bit for bit against torch indexing on every access width, the loader
against the stock DataLoader, no host synchronisation inside an epoch, and training / the synthesizer entry point giving
the same numbers with the switch on and off."""
import ctypes as C
import itertools
import os

import numpy as np
import pytest
import torch
from torch.utils.data import TensorDataset

from tests import parity_record

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CANARY = 0xA5
GUARD = 64            # canary bytes behind every destination


def _bytes(t):
    return t.contiguous().view(-1).view(torch.uint8)


def _launch(segs, idx, dst_offset=0):
    """One tl_gather_rows launch.  segs: [(src tensor (N, ...) on the GPU, channel list or None)].  Returns one uint8 tensor per
    segment (the gathered bytes) after checking the canary behind each destination and the error word."""
    from decode_tonal_langauge_amd import _lib
    lib = _lib.load()
    n = len(segs)
    src, dst, chan = (C.c_void_p * 4)(), (C.c_void_p * 4)(), (C.c_void_p * 4)()
    rows, n_c, inner, n_chan = (C.c_int64 * 4)(), (C.c_int64 * 4)(), (C.c_int64 * 4)(), (C.c_int64 * 4)()
    keep, bufs, sizes = [], [], []
    for k, (t, ch) in enumerate(segs):
        assert t.is_contiguous()
        sample = (t.numel() // t.shape[0]) * t.element_size()
        if ch is None:
            n_c[k], inner[k], n_chan[k], chan[k], out = 1, sample, 0, None, sample
        else:
            dev_ch = torch.tensor(ch, dtype=torch.int32, device=DEV)
            keep.append(dev_ch)
            n_c[k], inner[k], n_chan[k], chan[k] = t.shape[1], sample // t.shape[1], len(ch), dev_ch.data_ptr()
            out = len(ch) * (sample // t.shape[1])
        nbytes = out * idx.numel()
        buf = torch.full((dst_offset + nbytes + GUARD,), CANARY, dtype=torch.uint8, device=DEV)
        src[k], dst[k], rows[k] = t.data_ptr(), buf.data_ptr() + dst_offset, t.shape[0]
        bufs.append(buf)
        sizes.append(nbytes)
    err = torch.zeros(1, dtype=torch.int32, device=DEV)
    _lib.check(lib.tl_gather_rows(src, dst, rows, n_c, inner, chan, n_chan, n, idx.data_ptr(), idx.numel(), err.data_ptr(),
                                  _lib.stream_ptr()), "tl_gather_rows")
    torch.cuda.synchronize()
    assert int(err.item()) == 0
    got = []
    for buf, nbytes in zip(bufs, sizes):
        assert bool((buf[:dst_offset] == CANARY).all()) and bool((buf[dst_offset + nbytes:] == CANARY).all()), "canary overwritten"
        got.append(buf[dst_offset:dst_offset + nbytes].clone())
    return got


def _expect(t, ch, idx):
    ref = t[idx] if ch is None else t[idx][:, torch.tensor(ch, device=t.device)]
    return _bytes(ref)


def _source(shape, dtype, offset_elems=0, seed=0):
    """Random tensor of ``shape``; offset_elems > 0: a contiguous view that starts that many elements into its storage."""
    g = torch.Generator().manual_seed(seed)
    numel = int(np.prod(shape)) + offset_elems
    if dtype.is_floating_point:
        base = torch.randn(numel, generator=g, dtype=dtype)
    else:
        base = torch.randint(0, 200, (numel,), generator=g, dtype=dtype)
    return base.to(DEV)[offset_elems:].view(shape)


N_SRC, N_CH = 37, 6
# (dtype, shape after the sample dimension, bytes of one innermost row)
ROW_CASES = [
    pytest.param(torch.float32, (N_CH, 400), 1600, id="fp32-T400-1600B"),
    pytest.param(torch.float32, (N_CH, 5), 20, id="fp32-T5-20B"),
    pytest.param(torch.int64, (), 8, id="int64-label-8B"),
    pytest.param(torch.float32, (), 4, id="fp32-label-4B"),
    pytest.param(torch.uint8, (N_CH, 3), 3, id="uint8-T3-3B"),
]
CHANNEL_LISTS = [None, [3, 5, 0, 2, 4, 1], [4, 1, 5, 1, 0], [2], list(range(N_CH))]     # none, permuted, non-monotone, one, all


@pytest.mark.parametrize("dtype,tail,inner_bytes", ROW_CASES)
def test_gather_matches_torch_indexing_bit_for_bit(dtype, tail, inner_bytes):
    lists = CHANNEL_LISTS if tail else [None]
    g = torch.Generator().manual_seed(1)
    for offset in (0, max(1, 4 // torch.empty((), dtype=dtype).element_size())):
        # a view 4 bytes into its storage (int64: 8 bytes): every row starts off 16-byte alignment -> the 4-byte and byte paths
        src = _source((N_SRC,) + tail, dtype, offset_elems=offset, seed=2)
        assert src.data_ptr() % 16 == (offset * src.element_size()) % 16
        if tail:
            assert src.shape[2] * src.element_size() == inner_bytes
        else:
            assert src.element_size() == inner_bytes
        for n_idx in (1, 63, 64, 65, 257):
            idx = torch.randint(0, N_SRC, (n_idx,), generator=g).to(DEV)               # 257 draws of 37 rows: repeats
            for ch in lists:
                got, = _launch([(src, ch)], idx)
                assert torch.equal(got, _expect(src, ch, idx)), (offset, n_idx, ch)
    # a destination that starts 4 bytes / 1 byte off alignment
    idx = torch.tensor([5, 5, 0, N_SRC - 1, 5], device=DEV)
    for dst_offset in (4, 1):
        for ch in lists:
            got, = _launch([(src, ch)], idx, dst_offset=dst_offset)
            assert torch.equal(got, _expect(src, ch, idx)), (dst_offset, ch)


def test_four_segments_in_one_launch():
    ecog = _source((N_SRC, N_CH, 400), torch.float32, seed=3)
    odd = _source((N_SRC, N_CH, 5), torch.float32, offset_elems=1, seed=4)
    label = _source((N_SRC,), torch.int64, seed=5)
    small = _source((N_SRC, N_CH, 3), torch.uint8, seed=6)
    segs = [(ecog, [5, 0, 3]), (odd, None), (label, None), (small, [1, 1, 4, 0])]
    g = torch.Generator().manual_seed(7)
    for n_idx in (1, 65, 257):
        idx = torch.randint(0, N_SRC, (n_idx,), generator=g).to(DEV)
        together = _launch(segs, idx)
        for (t, ch), got in zip(segs, together):
            alone, = _launch([(t, ch)], idx)
            assert torch.equal(got, alone) and torch.equal(got, _expect(t, ch, idx)), (n_idx, ch)
    # the same source read through two lists and whole (ecog stored once, three views of it)
    idx = torch.arange(N_SRC - 1, -1, -1, device=DEV)
    three = _launch([(ecog, [0, 1]), (ecog, [4]), (ecog, None)], idx)
    for (ch, got) in zip(([0, 1], [4], None), three):
        assert torch.equal(got, _expect(ecog, ch, idx))


# ------------------------------------------------------------------------------------------------ loader
RATIOS, SHUFFLE, LISTS = [0.74, 0.15, 0.11], [True, False, False], ([4, 0, 6], [5, 2])


def _fields():
    g = torch.Generator().manual_seed(11)
    x = torch.randn(203, 7, 25, generator=g)
    y = torch.randn(203, 3, 4, generator=g)
    z = torch.randn(203, 11, generator=g)
    return x, y, z


def _resident_loaders(seed=7):
    from decode_tonal_langauge_amd.data_loading.dataloaders import split_dataset
    from decode_tonal_langauge_amd.data_loading.resident import ResidentDataset
    x, y, z = _fields()
    rds = ResidentDataset([(x, LISTS[0]), (x, LISTS[1]), (y, None), (z, None)], device=DEV)
    assert rds._tensors[0] is rds._tensors[1] and rds._tensors[0].is_cuda                  # stored once
    return split_dataset(rds, RATIOS, SHUFFLE, batch_size=16, seed=seed, resident=True)


def test_loader_yields_the_stock_loaders_batches():
    from decode_tonal_langauge_amd.data_loading.dataloaders import split_dataset
    x, y, z = _fields()
    stock = split_dataset(TensorDataset(x[:, LISTS[0]], x[:, LISTS[1]], y, z), RATIOS, SHUFFLE, batch_size=16, seed=7)
    want, states = [], []
    for _epoch in range(2):
        want.append([[b for b in loader] for loader in stock])
        states.append(torch.get_rng_state())
    resident = _resident_loaders(seed=7)
    assert [len(l) for l in resident] == [len(l) for l in stock] == [10, 2, 2]
    for epoch in range(2):
        for loader, batches in zip(resident, want[epoch]):
            got = list(loader)
            assert len(got) == len(batches) and [len(b[0]) for b in got][-1] in (150 % 16, 30 % 16, 23 % 16)   # ragged tail
            for gb, sb in zip(got, batches):
                assert len(gb) == 4
                for gt, st in zip(gb, sb):
                    assert gt.is_cuda and gt.dtype == st.dtype and gt.shape == st.shape and torch.equal(gt.cpu(), st)
        assert torch.equal(torch.get_rng_state(), states[epoch])


def test_no_host_sync_between_the_batches_of_an_epoch():
    loader = _resident_loaders()[0]
    list(loader)                                       # the subset goes up with the first epoch
    it = iter(loader)
    first = next(it)                                   # this epoch's order is uploaded here
    rest = []
    mode = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        for _ in range(len(loader) - 1):
            rest.append(next(it))
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    assert next(it, None) is None                      # exhausting the iterator reads the error word: the one sync
    assert len(rest) == 9 and first[0].shape == (16, 3, 25) and rest[-1][0].shape == (150 % 16, 3, 25)
    order = torch.as_tensor(list(itertools.chain.from_iterable(loader.sampler.batches)))
    x = _fields()[0]
    assert torch.equal(torch.cat([first[1]] + [b[1] for b in rest]).cpu(), x[order][:, LISTS[1]])


def test_training_through_the_resident_loader_is_the_same_training(tmp_path):
    from decode_tonal_langauge_amd.data_loading.dataloaders import split_dataset
    from decode_tonal_langauge_amd.models.classifier_trainer import ClassifierTrainer
    from decode_tonal_langauge_amd.models.simple_classifiers import LogisticRegressionClassifier
    g = torch.Generator().manual_seed(21)
    labels = torch.randint(0, 4, (128,), generator=g)
    feats = torch.randn(128, 16, 100, generator=g) + labels[:, None, None].float() * 0.3
    tds = TensorDataset(feats.to(DEV), labels.float().to(DEV))          # what prepare_torch_dataset hands the pipeline

    def fit(resident):
        torch.manual_seed(5)
        loaders = split_dataset(tds, [0.75, 0.25], [True, False], batch_size=32, seed=5, resident=resident)
        assert len(loaders[0]) == 3                                     # 96 training samples at batch 32
        model = LogisticRegressionClassifier(16 * 100, 4).to(DEV)
        trainer = ClassifierTrainer(model, 0.005, 0.01, log_dir=str(tmp_path / str(resident)), fused=True)
        hist = trainer.fit(loaders[0], loaders[1], max_epochs=2, patience=99)
        pred = trainer.predict(loaders[1]).cpu()
        return {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}, hist, pred, torch.get_rng_state()

    sd0, h0, p0, r0 = fit(False)
    sd1, h1, p1, r1 = fit(True)
    assert len(h0) == 2 and h0 == h1                                    # the history rows, float for float
    assert sd0.keys() == sd1.keys() and all(torch.equal(sd0[k], sd1[k]) for k in sd0)
    assert torch.equal(p0, p1) and torch.equal(r0, r1)


def test_train_synthesizer_with_and_without_resident(tmp_path, monkeypatch):
    """``train_synthesizer.run`` three times from one seed: without the key, with ``resident: false``, with ``resident: true``.
    The evaluation targets are bitwise equal.  The per-epoch losses of the resident run are held to what two stock runs differ
    by.  Observed on an MI355X: the first stock run of the process differs from the second by 4.1e-4 in the epoch loss, the
    resident run (third) equals the second stock run exactly and so differs from the first by the same 4.1e-4
    (``profiles/parity_observed.json``, section ``resident_loader_entry_point``)."""
    from decode_tonal_langauge_amd import train_synthesizer as ts
    from decode_tonal_langauge_amd.data_loading import synthetic
    channels = {"active_channels": list(range(24)), "tone_discriminative": [0, 1, 2, 3], "syllable_discriminative": [4, 5, 6, 7]}
    written = synthetic.write_dataset(str(tmp_path / "data"), channels=channels, n_samples=48, n_channels=24, n_timepoints=200)
    seen = {}
    train, evaluate = ts.train, ts.SynthesisTrainer.evaluate
    monkeypatch.setattr(ts, "train", lambda params: seen.setdefault("row", train(params)))

    def recording_evaluate(self, loader):
        got = evaluate(self, loader)
        seen["eval"] = (type(loader).__name__,) + tuple(got)
        return got
    monkeypatch.setattr(ts.SynthesisTrainer, "evaluate", recording_evaluate)

    def run(tag, resident):
        seen.clear()
        params = dict(sample_path=os.path.join(written["sample_dir"], "subject_1.npz"), subject_id="1",
                      result_file=str(tmp_path / tag / "results.csv"),
                      channel_file=os.path.join(written["channel_selection_dir"], "subject_1.json"),
                      config_file=written["config_file"], model_name="lite-resident", synthesis_model_name="SynthesisLite",
                      syllable_model_name="logistic", tone_model_name="logistic", device=DEV, batch_size=8, epochs=2,
                      repeat=1, verbose=0, seed=3)
        if resident is not None:
            params["resident"] = resident
        ts.run({"training": {"params": params}})
        kind, _mcd, recon, origin = seen["eval"]
        assert kind == ("ResidentLoader" if resident else "DataLoader")
        losses = np.asarray(seen["row"]["losses"][0], dtype=np.float64)
        assert losses.shape == (2,) and np.isfinite(losses).all()
        return origin, recon, losses

    o_a, _r_a, l_a = run("a", None)              # the default: the key is absent
    o_b, _r_b, l_b = run("b", False)
    o_r, _r_r, l_r = run("r", True)
    assert o_a.shape == (5, 80) and np.array_equal(o_a, o_b) and np.array_equal(o_a, o_r)          # bitwise
    stock_vs_stock = float(np.abs(l_a - l_b).max())
    resident_vs_stock = float(np.abs(l_r - l_a).max())
    resident_vs_second = float(np.abs(l_r - l_b).max())
    parity_record.record("resident_loader_entry_point", {"loss_stock_vs_stock": stock_vs_stock,
                                                         "loss_resident_vs_stock": resident_vs_stock,
                                                         "loss_resident_vs_second_stock": resident_vs_second})
    print(f"per-epoch loss: stock vs stock {stock_vs_stock:.3e}, resident vs stock {resident_vs_stock:.3e} "
          f"(vs the second stock run {resident_vs_second:.3e})")
    # identical batches: the resident run may differ from a stock run by no more than two stock runs differ from each other
    assert resident_vs_stock <= stock_vs_stock, (l_a.tolist(), l_b.tolist(), l_r.tolist())


def test_classifier_pipeline_key(tmp_path, monkeypatch):
    """``training.params.resident`` of ``train_classifier``: the resident loaders reach the trainer and the results row
    (the metrics of every seed) is the one of the stock loaders."""
    import pandas as pd
    from decode_tonal_langauge_amd import train_classifier
    from decode_tonal_langauge_amd.data_loading import synthetic
    from decode_tonal_langauge_amd.models import classifier_trainer as ct
    written = synthetic.write_dataset(str(tmp_path / "data"), n_samples=120, n_channels=8, n_timepoints=50)
    kinds = []
    fit = ct.ClassifierTrainer.fit

    def recording_fit(self, train_loader, val_loader, **kw):
        kinds.append((type(train_loader).__name__, type(val_loader).__name__, len(train_loader)))
        return fit(self, train_loader, val_loader, **kw)
    monkeypatch.setattr(ct.ClassifierTrainer, "fit", recording_fit)

    def run(resident):
        config = {
            "model": {"model": "models.simple_classifiers.LogisticRegressionClassifier", "model_name": "logistic"},
            "dataset": {"class_labels": {"tone": None}},
            "training": {"module": "train_classifier", "params": {
                "fused": True, "resident": resident,
                "io": {"log_dir": str(tmp_path / f"logs_{resident}"), "sample_dir": written["sample_dir"],
                       "channel_selection_dir": written["channel_selection_dir"]},
                "experiment": {"targets": ["tone"], "features": "ecog", "separate_models": False, "seed": 1, "repeat": 2,
                               "verbose": 0, "device": DEV},
                "training": {"train_ratio": 0.75, "vali_ratio": 0.125, "test_ratio": 0.125, "batch_size": 32, "epochs": 2,
                             "lr": 0.005, "patience": 5, "weight_decay": 0.01, "log_every_n_steps": 10}}},
            "evaluation": {"metrics": ["accuracy", "f1_score"]},
        }
        row = pd.read_csv(os.path.join(train_classifier.run(config), "results.csv")).iloc[0]
        return {k: row[k] for k in row.index if k.startswith(("accuracy", "f1")) or k == "seeds"}

    stock, resident = run(False), run(True)
    assert kinds == [("DataLoader", "DataLoader", 3)] * 2 + [("ResidentLoader", "ResidentLoader", 3)] * 2
    assert stock == resident, (stock, resident)


def test_dataset_that_does_not_fit_is_refused(monkeypatch):
    from decode_tonal_langauge_amd.data_loading.resident import ResidentDataset
    x, y, _z = _fields()
    monkeypatch.setattr(torch.cuda, "mem_get_info", lambda device=None: (1000, 1 << 30))
    need = x.numel() * 4 + y.numel() * 4                      # x counts once although two fields read it
    with pytest.raises(RuntimeError, match=f"needs {need} bytes"):
        ResidentDataset([(x, LISTS[0]), (x, LISTS[1]), (y, None)], device=DEV)
