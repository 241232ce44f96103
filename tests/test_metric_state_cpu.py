"""What the seven Trainer metrics pickle: ``__getstate__`` / ``__setstate__`` against states recorded before the metrics shared
one state rule.  Checkpoints of earlier runs hold these dictionaries, so they must stay key for key and value for value.

tests/golden/metric_states.json was written once, from the commit before the shared rule, by

    import json, tests.test_metric_state_cpu as T
    json.dump({name: m.__getstate__() for name, m in T.metrics().items()}, open(T.GOLDEN, "w"), indent=1, sort_keys=True)

(JSON stores the one tuple among the values, TissueYield's ``percentiles``, as a list; the comparison goes through the same
conversion).  No device is needed: the tensors are 8 tiles of 32 x 32 and nothing is evaluated.
"""
import json
import os
from types import SimpleNamespace

import pytest
import torch

from rna_gan_amd import metrics as M

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "metric_states.json")
ENCODING_DIMS = 4

# per class: the one history entry, and every attribute that is dropped on pickling and comes back as None
HISTORY = {
    "PrecisionRecall": {"precision": 0.5, "recall": 0.25, "density": 0.75, "coverage": 0.125},
    "TissueYield": {"accepted": 0.5, "tissue_fraction": 0.375, "low_contrast": 0.125},
    "ConditioningFidelity": {"top1": 0.5, "top5": 1.0, "mrr": 0.625, "median_rank": 1.5, "chance_top1": 0.25},
    "Memorisation": {"copy_rate": 0.5, "exact": 0.0, "min_d2": 3, "median_d2": 8.0},
    "PairDiversity": {"generated": 0.5, "real": 0.25, "gap": 0.25, "per_scale": [[0.5, 0.375], [0.625, 0.5]]},
}
DROPPED = {
    "FrechetDistance": ("noise", "real", "_real_stats"),
    "KernelDistance": ("noise", "real", "_real_stats", "last"),
    "PrecisionRecall": ("noise", "real", "_real_stats", "_real_radii", "last"),
    "TissueYield": ("noise", "last", "last_stats"),
    "ConditioningFidelity": ("real_tiles", "patient_of", "rna", "betavae", "_real_centroids", "last", "last_rank"),
    "Memorisation": ("noise", "train_tiles", "heldout", "_index", "last", "last_result"),
    "PairDiversity": ("noise", "real", "_real_score", "last", "last_scores"),
}
NAMES = tuple(DROPPED)


def metrics():
    """{class name: the metric}, each with fixed non-default settings, a renamed argument and (where it keeps one) one history
    entry; the noise of the classes that draw it is drawn at construction"""
    tiles = (torch.arange(8 * 3 * 32 * 32, dtype=torch.int64) * 37 % 256).to(torch.uint8).reshape(8, 3, 32, 32)
    rna = torch.arange(4 * 5, dtype=torch.float32).reshape(4, 5) / 8.0
    patient_of = torch.arange(8, dtype=torch.int32) % 4
    out = {
        "FrechetDistance": M.FrechetDistance(tiles, n_fake=6, extractor=lambda x: x, seed=11, batch_size=3, encoding_dims=ENCODING_DIMS),
        "KernelDistance": M.KernelDistance(tiles, n_fake=5, seed=12, batch_size=4, encoding_dims=ENCODING_DIMS, num_subsets=3,
                                           subset_size=4, degree=2, gamma=0.25, coef0=0.5),
        "PrecisionRecall": M.PrecisionRecall(tiles, n_fake=7, extractor=lambda x: x, seed=13, batch_size=5,
                                             encoding_dims=ENCODING_DIMS, nearest_k=3, report="density"),
        "TissueYield": M.TissueYield(6, min_tissue=0.25, rgb_min=40, dilate=2, percentiles=(2, 97.5), fraction=0.0625,
                                     luma_range=3.0, seed=14, batch_size=2, encoding_dims=ENCODING_DIMS),
        "ConditioningFidelity": M.ConditioningFidelity(tiles, patient_of, rna, None, tiles_per_patient=3, seed=15, batch_size=6,
                                                       center=False, report="mrr", group=64),
        "Memorisation": M.Memorisation(tiles, 5, factor=2, k=3, d4=True, heldout=tiles[:2], seed=16, batch_size=3,
                                       encoding_dims=ENCODING_DIMS),
        "PairDiversity": M.PairDiversity(6, pairs=4, real=tiles, scales=2, seed=17, batch_size=4, encoding_dims=ENCODING_DIMS),
    }
    for name, m in out.items():
        m.set_arg_map({"generator": "generator_ema"})
        if name in HISTORY:
            m.history.append(json.loads(json.dumps(HISTORY[name])))
    return out


@pytest.fixture(scope="module")
def built():
    with open(GOLDEN) as f:
        return metrics(), json.load(f)


def test_every_metric_is_covered(built):
    live, golden = built
    assert set(live) == set(golden) == set(NAMES)
    assert [n for n in NAMES if issubclass(getattr(M, n), M.EvaluationMetric)] == list(NAMES)


@pytest.mark.parametrize("name", NAMES)
def test_state_is_the_recorded_one(built, name):
    live, golden = built
    state = live[name].__getstate__()
    assert json.loads(json.dumps(state)) == golden[name]                  # dictionaries: the order of the keys is free, the values are not
    assert set(state) == set(golden[name]) and ("history" in state) == (name in HISTORY)
    assert state["arg_map"] == {"generator": "generator_ema"} and state["arg_map"] is not live[name].arg_map
    assert all(not torch.is_tensor(v) and not callable(v) for v in state.values()), "settings only"
    if name == "TissueYield":
        assert state["percentiles"] == (2.0, 97.5) and isinstance(state["percentiles"], tuple)
    if "extractor" in state:
        assert state["extractor"] == ("discriminator" if name in ("KernelDistance", "ConditioningFidelity") else "callable")


@pytest.mark.parametrize("name", NAMES)
def test_setstate_restores_settings_and_drops_the_rest(built, name):
    live, _ = built
    cls, state = type(live[name]), live[name].__getstate__()
    given = {k: v for k, v in reversed(list(state.items()))}              # another key order
    back = cls.__new__(cls)
    back.__setstate__(given)
    for attr in DROPPED[name]:
        assert hasattr(back, attr) and getattr(back, attr) is None, attr
    for key, value in state.items():
        assert getattr(back, key) == value, key
    assert back.__getstate__() == state
    if name in HISTORY:
        assert back.history == given["history"] == [HISTORY[name]] and back.history is not given["history"]
        assert back.history[0] is not given["history"][0]
        assert live[name].__getstate__()["history"][0] is not live[name].history[0]
    else:
        assert not hasattr(back, "history")


@pytest.mark.parametrize("name", [n for n in NAMES if n != "ConditioningFidelity"])
def test_unpickled_metric_draws_the_noise_of_its_seed(built, name):
    live, _ = built
    m = live[name]
    back = type(m).__new__(type(m))
    back.__setstate__(m.__getstate__())
    drawn = back._noise_for(SimpleNamespace(encoding_dims=ENCODING_DIMS), "cpu")
    assert drawn.shape == (m.n_fake, ENCODING_DIMS) and torch.equal(drawn, m.noise)
    assert torch.equal(drawn, torch.randn(m.n_fake, ENCODING_DIMS, generator=torch.Generator().manual_seed(m.seed)))
    assert back._noise_for(SimpleNamespace(encoding_dims=ENCODING_DIMS), "cpu") is not None and torch.equal(back.noise, drawn)
