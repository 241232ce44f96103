"""Dynamic loss scaling (rna_gan_amd.amp) without a GPU: the GradScaler update rule, the state_dict keys, and the constructor's
refusal of anything but powers of two."""
import pytest

from rna_gan_amd.amp import DynamicLossScaler


def test_update_rule_matches_gradscaler():
    rule = DynamicLossScaler.update_rule
    # three clean steps with growth_interval 3: the third doubles and resets the tracker
    st = (12, 0, 0)
    st = rule(*st, False, 3, 0, 24); assert st == (12, 1, 0)
    st = rule(*st, False, 3, 0, 24); assert st == (12, 2, 0)
    st = rule(*st, False, 3, 0, 24); assert st == (13, 0, 0)
    # a non-finite step halves, resets the tracker, counts the skip
    st = rule(12, 2, 5, True, 3, 0, 24); assert st == (11, 0, 6)
    # caps
    assert rule(0, 0, 0, True, 3, 0, 24) == (0, 0, 1)
    assert rule(24, 2, 0, False, 3, 0, 24) == (24, 0, 0)


def test_state_dict_keys_and_round_trip():
    sc = DynamicLossScaler(init_scale=2.0 ** 10, growth_interval=7)
    sd = sc.state_dict()
    assert set(sd) == {"scale", "growth_factor", "backoff_factor", "growth_interval", "_growth_tracker", "skipped_steps"}
    assert sd["scale"] == 1024.0 and sd["growth_interval"] == 7 and sd["_growth_tracker"] == 0 and sd["skipped_steps"] == 0
    other = DynamicLossScaler()
    other.load_state_dict(dict(sd, scale=2.0 ** 15, _growth_tracker=3, skipped_steps=9))
    got = other.state_dict()
    assert got["scale"] == 2.0 ** 15 and got["_growth_tracker"] == 3 and got["skipped_steps"] == 9 and got["growth_interval"] == 7


def test_defaults():
    sd = DynamicLossScaler().state_dict()
    assert sd["scale"] == 4096.0 and sd["growth_interval"] == 2000
    sc = DynamicLossScaler()
    assert sc.min_exp == 0 and sc.max_exp == 24


@pytest.mark.parametrize("kw", [{"init_scale": 3000.0}, {"min_scale": 0.3}, {"max_scale": 1e6}, {"growth_factor": 4.0},
                                {"backoff_factor": 0.25}, {"growth_factor": 1.5}, {"growth_interval": 0},
                                {"min_scale": 2.0 ** 10, "max_scale": 2.0 ** 5}, {"init_scale": -2.0}])
def test_rejects_bad_arguments(kw):
    with pytest.raises(ValueError):
        DynamicLossScaler(**kw)


def test_load_rejects_other_factors():
    with pytest.raises(ValueError):
        DynamicLossScaler().load_state_dict({"scale": 8.0, "growth_factor": 3.0, "backoff_factor": 0.5})


def test_cli_accepts_dynamic_for_fp16_only():
    """histopathology_gan.py refuses --loss_scaling dynamic with another precision, and an unknown mode, before touching a GPU."""
    import os
    import subprocess
    import sys
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cli = [sys.executable, os.path.join(repo, "histopathology_gan.py"), "--config", os.path.join(repo, "configs",
                                                                                                 "gan_run_synthetic.json")]
    for extra, msg in ((["--precision", "bf16", "--loss_scaling", "dynamic"], "fp16 only"),
                       (["--precision", "fp16", "--loss_scaling", "sometimes"], "static or dynamic")):
        r = subprocess.run(cli + extra, capture_output=True, text=True, timeout=300)
        assert r.returncode != 0 and msg in r.stderr, r.stderr[-1000:]
