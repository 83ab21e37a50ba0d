"""`train.ValidationLoop` on the MI355X: the reference's three validation hooks (train.py:118-160) around the tiny / tiny tokenizer.
Two batches of two clips with different shapes and token counts, 'psnr' and 'ssim', two logged clips out of four.  `-m gpu`."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from titok_video_amd.model.metrics.eval_metrics import EvalMetrics
from titok_video_amd.model.titok import TiTok
from titok_video_amd.synthetic import seeded_titok_state, synthetic_clips
from titok_video_amd.train import ValidationLoop, recon_panels

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LEVELS = [7, 5, 5, 5, 5]
SHAPES = [[(4, 16, 16), (8, 16, 24)], [(4, 16, 24), (4, 16, 16)]]
COUNTS = [[3, 6], [2, 5]]
FPS = [[8, 12.5], [24, 30]]


def config():
    return SimpleNamespace(tokenizer=SimpleNamespace(model=SimpleNamespace(patch_size=[4, 8, 8], fsq_levels=LEVELS, encoder_size="tiny",
                                                                           decoder_size="tiny")),
                           training=SimpleNamespace(eval=SimpleNamespace(log_metrics=["psnr", "ssim"])))


@pytest.fixture(scope="module")
def setup():
    """The model, the two batches, and what the model gives for them - computed once and left alone."""
    model = TiTok(config())
    model.load_state_dict(seeded_titok_state(0), strict=True)
    model = model.to(DEV, torch.float32).eval()
    batches = []
    for k, (shapes, counts, fps) in enumerate(zip(SHAPES, COUNTS, FPS)):
        clips = synthetic_clips(shapes, seed=20 + k, dtype=torch.float32, device=DEV)
        batches.append({"video": clips, "fps": fps if k == 0 else torch.tensor(fps), "token_counts": counts if k == 0 else torch.tensor(counts)})
    with torch.no_grad():
        recons = [model(b["video"], b["token_counts"])[0] for b in batches]
    direct = EvalMetrics(config())
    for b, r in zip(batches, recons):
        direct.update(r, b["video"])
    want_metrics = direct.compute()
    torch.cuda.synchronize()
    return model, batches, recons, want_metrics


class _Codebook:
    def __init__(self, ready):
        self.ready, self.asked = ready, 0

    def is_score_ready(self):
        return self.ready

    def get_scores(self):
        self.asked += 1
        return {"codebook/usage_percent": 12.5, "codebook/entropy": 1.25}


def run_epoch(loop, batches):
    loop.start()
    logged, seen = [], []
    for b in batches:
        logged.append(loop.step(b))
        seen.append((loop.seen_eval, loop.seen_recon))
    return logged, seen, loop.end()


@pytest.mark.parametrize("random_recon", [False, True])
def test_validation_epoch(setup, random_recon):
    model, batches, recons, want_metrics = setup
    metrics = EvalMetrics(config())
    loop = ValidationLoop(model, metrics, log_recon_num=2, eval_samples=4, random_recon=random_recon)
    torch.manual_seed(5)
    want_idx = torch.randperm(4)[:2].tolist() if random_recon else [0, 1]
    torch.manual_seed(5)
    logged, seen, got_metrics = run_epoch(loop, batches)
    assert loop.recon_indexes == want_idx
    # the running index counts every clip, selected or not; the logged ones are numbered from 1 in the order they are met
    assert [s[0] for s in seen] == [2, 4]
    flat_clips = [(b, i) for b in range(2) for i in range(2)]
    picked = [k for k in range(4) if k in want_idx]
    assert [len(l) for l in logged] == [sum(1 for k in picked if k // 2 == b) for b in range(2)]
    assert seen[-1][1] == 2
    entries = [e for l in logged for e in l]
    for n, (k, e) in enumerate(zip(picked, entries), start=1):
        b, i = flat_clips[k]
        assert set(e) == {"key", "video", "fps", "caption"}
        assert e["key"] == f"Video recon {n}"
        assert e["caption"] == f"{COUNTS[b][i]} tokens"
        assert e["fps"] == FPS[b][i] and not torch.is_tensor(e["fps"])
        (want,) = recon_panels([batches[b]["video"][i]], [recons[b][i]])
        T, H, W = SHAPES[b][i]
        assert e["video"].dtype == np.uint8 and e["video"].shape == (T, 3, H, 2 * W)
        assert np.array_equal(e["video"], want), (b, i)
    # exactly what an EvalMetrics fed the same reconstructions returns; and the metrics were reset
    assert got_metrics == want_metrics and set(got_metrics) == {"eval/psnr", "eval/ssim"}
    assert float(metrics._acc.abs().sum()) == 0.0 and float(metrics._ssim_acc.abs().sum()) == 0.0
    # a second start() puts the counters back: the same epoch again gives the same keys, panels and metrics
    torch.manual_seed(5)
    logged2, seen2, got2 = run_epoch(loop, batches)
    assert seen2 == seen and got2 == want_metrics
    entries2 = [e for l in logged2 for e in l]
    assert [e["key"] for e in entries2] == [e["key"] for e in entries]
    assert all(np.array_equal(a["video"], b["video"]) for a, b in zip(entries, entries2))


def test_codebook_scores_are_merged_when_ready(setup):
    model, batches, recons, want_metrics = setup
    for ready in (False, True):
        cb = _Codebook(ready)
        loop = ValidationLoop(model, EvalMetrics(config()), log_recon_num=0, eval_samples=4, random_recon=False, codebook_logger=cb)
        logged, seen, got = run_epoch(loop, batches)
        assert logged == [[], []] and seen == [(2, 0), (4, 0)]
        want = dict(want_metrics)
        if ready:
            want.update(cb.get_scores())
        assert got == want and cb.asked == (2 if ready else 0)
