"""GPU: a plain bench.py run (no --full) on a small shape, in process — the result line's headline
fields, and --dump-outputs: the model after the last timed step, the same from run to run and equal to
the one the same next() calls give through the API."""
import json
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402

D, T, V, K, STEPS, WARMUP = 4000, 30, 4096, 16, 2, 1
ARGS = ["--gpus", "1", "--steps", str(STEPS), "--warmup", str(WARMUP), "--docs", str(D), "--tokens", str(T),
        "--vocab", str(V), "--k", str(K), "--workers", "1"]


def _run(monkeypatch, capsys, out, ctx):
    import stc

    monkeypatch.delenv("WORLD_SIZE", raising=False)
    monkeypatch.setattr(stc, "Context", lambda device: ctx)  # the suite's context, not one more per run
    monkeypatch.setattr(sys, "argv", ["bench.py"] + ARGS + ["--dump-outputs", str(out)])
    bench.main()
    return json.loads(capsys.readouterr().out.strip().splitlines()[-1])


@pytest.mark.gpu
def test_plain_run_line_and_reproducible_dump(ctx, monkeypatch, capsys, tmp_path):
    import stc
    from stc import synth

    line = _run(monkeypatch, capsys, tmp_path / "a", ctx)
    assert line["metric"] == bench.METRIC and line["unit"] == "docs/s" and line["higher_is_better"] is True
    assert line["dtype"] == "f64" and line["steps"] == STEPS and line["warmup"] == WARMUP
    assert line["ms_per_step"] > 0
    # value and ms_per_step describe the same timed steps: docs of the steps ÷ their wall time
    docs = line["value"] * line["ms_per_step"] * 1e-3 * STEPS
    assert docs == pytest.approx(round(docs), abs=1e-6) and 0.5 * 0.05 * D * STEPS < docs < 1.5 * 0.05 * D * STEPS
    assert line["secondary"] == [] and line["cpu_baseline"] is None
    assert line["roofline"]["hbm_copy_measured_GBs"] is None
    lam, alpha = np.load(tmp_path / "a" / "topics.npy"), np.load(tmp_path / "a" / "alpha.npy")
    assert lam.dtype == np.float64 and lam.shape == (V, K) and alpha.dtype == np.float64 and alpha.shape == (K,)
    assert np.all(np.isfinite(lam)) and np.all(lam > 0) and np.all(alpha > 0)

    _run(monkeypatch, capsys, tmp_path / "b", ctx)
    assert np.array_equal(lam, np.load(tmp_path / "b" / "topics.npy"))
    assert np.array_equal(alpha, np.load(tmp_path / "b" / "alpha.npy"))

    # the same corpus, seed and number of next() calls through the API: 20 untimed minibatches, then --steps
    monkeypatch.setattr(sys, "argv", ["bench.py"] + ARGS)
    a = bench.parse()
    corpus = synth.make_corpus(a.corpus, D, T, V, K, a.seed, 0, D, 1)
    h = stc.LdaHandle(ctx, K, V, mini_batch_fraction=a.fraction, optimize_doc_concentration=True, seed=a.seed,
                      dtype="f64")
    dc = stc.DeviceCsr.upload(ctx, corpus, stc.STC_F64)
    h.set_corpus(dc, D)
    h.init_random(a.seed)
    for _ in range(a.state_minibatches + STEPS):
        h.next(stats=False)
    assert np.array_equal(h.topics(), lam) and np.array_equal(h.alpha(), alpha)
    h.close()
    dc.free()
