"""Pins tests/ema_refs.py, the bit-exact numpy reference of rg_ema_update that the GPU tests compare against: against the closed
form in fp64 with counted roundings, against an independent implementation (torch.optim.swa_utils), the warm-up formula at exact
points, the fixed point; and the launcher's --g_ema / --g_ema_warmup flags.  No GPU."""
import sys

import numpy as np
import pytest
import torch
import torch.nn as nn

from ema_refs import F32, decay_at, ema_closed_form, ema_closed_form_bound, ema_update_ref


@pytest.mark.parametrize("decay", [0.5, 0.9, 0.999, 0.9999])
@pytest.mark.parametrize("warm", [False, True])
def test_closed_form_for_constant_p(decay, warm):
    """50 updates towards a constant p: e_k = p + (e0 - p) d^k (d_t under warm-up), within the counted roundings."""
    rng = np.random.default_rng(3)
    p = rng.normal(size=257).astype(np.float32)
    e0 = rng.normal(size=257).astype(np.float32)
    seq, decays = [e0], []
    for k in range(50):
        t = k + 1 if warm else None
        decays.append(float(decay_at(decay, t)))
        seq.append(ema_update_ref(p, seq[-1], decay, t))
    want = ema_closed_form(p, e0, decays)
    bound = ema_closed_form_bound(p, seq, decays)
    err = np.abs(seq[-1].astype(np.float64) - want)
    print("decay %g warm %s: max err %.3g, max bound %.3g" % (decay, warm, err.max(), bound.max()))
    assert np.all(err <= bound)
    # the bound itself is not a vacuous one: per update at most U32 (2 |p - e| + |e'|) <= 5 U32 M with M = max(|p|, |e0|)
    assert bound.max() <= 5 * 50 * 2.0 ** -24 * max(np.abs(p).max(), np.abs(e0).max())
    # and the average moved: after 50 updates at d <= 0.9 the start is forgotten to the rounding level
    if decay <= 0.9:
        assert np.abs(seq[-1] - p).max() <= 0.9 ** 50 * np.abs(e0 - p).max() + bound.max()


def test_against_swa_utils_averaged_model():
    """torch.optim.swa_utils.AveragedModel with the EMA averaging function: its first update COPIES, the later ones are
    lerp(e, p, 1 - 0.9) -- a differently rounded form of the same recurrence (the weight is fl32(0.1) instead of 1.f - fl32(0.9),
    and lerp may contract): at most 2 ulp apart per update, damped by d: 2 / (1 - d) = 20 ulp of max|value| in total."""
    from torch.optim.swa_utils import AveragedModel, get_ema_multi_avg_fn
    torch.manual_seed(0)
    m = nn.Linear(7, 5)
    avg = AveragedModel(m, multi_avg_fn=get_ema_multi_avg_fn(0.9))
    avg.update_parameters(m)                                       # the copy
    mine = [p.detach().numpy().copy() for p in m.parameters()]
    worst, top = 0.0, 0.0
    for _ in range(20):
        with torch.no_grad():
            for p in m.parameters():
                p.add_(0.05 * torch.randn_like(p))
        avg.update_parameters(m)
        mine = [ema_update_ref(p.detach().numpy(), e, 0.9) for p, e in zip(m.parameters(), mine)]
        for e, a in zip(mine, avg.module.parameters()):
            worst = max(worst, float(np.abs(e.astype(np.float64) - a.detach().numpy().astype(np.float64)).max()))
            top = max(top, float(np.abs(e).max()))
    bound = 20 * float(np.spacing(F32(top)))
    print("max |reference - AveragedModel| = %.3g, bound %.3g" % (worst, bound))
    assert worst <= bound
    assert any(not np.array_equal(e, p.detach().numpy()) for e, p in zip(mine, m.parameters()))     # it is an average, not a copy


def test_warmup_formula():
    for t, r in ((2, 0.25), (6, 0.4375), (8, 0.5), (26, 0.75)):
        assert decay_at(0.999, t) == F32(r) and decay_at(0.999, t).dtype == np.float32
        assert decay_at(0.125, t) == F32(0.125)                    # the cap wins below the ratio
    assert decay_at(0.999, None) == F32(0.999)
    # once the ratio exceeds the decay the decay is used as is: (1 + t) / (10 + t) > 0.999 <=> t > 8989
    assert decay_at(0.999, 8989) < F32(0.999)
    for t in (8991, 10 ** 6, 2 ** 31 - 1):
        assert decay_at(0.999, t) == F32(0.999)
    assert decay_at(0.9999, 10 ** 6) == F32(0.9999)
    ds = [float(decay_at(0.9999, t)) for t in list(range(1, 3000)) + [10 ** 4, 10 ** 5, 10 ** 6, 10 ** 7]]
    assert all(a <= b for a, b in zip(ds, ds[1:])) and ds[0] == float(F32(2.0) / F32(11.0))
    assert decay_at(0.0, 5) == F32(0.0)


def test_fixed_point_and_extremes():
    rng = np.random.default_rng(5)
    p = np.concatenate([rng.normal(size=64), [0.0, 1e-45, -1e-45, 1e-39, 3e38, -3e38, 1.0, -1.0]]).astype(np.float32)
    for decay, t in ((0.999, None), (0.5, None), (0.9999, 3), (0.0, None)):
        out = ema_update_ref(p, p.copy(), decay, t)
        assert out.tobytes() == p.tobytes()                         # e == p: bit-identical (denormals and +0 included)
    # (-0) is the one exception: (-0) - (-0) = +0 and (-0) + (+0) = +0 in IEEE arithmetic
    z = ema_update_ref(np.array([-0.0], np.float32), np.array([-0.0], np.float32), 0.5)
    assert z[0] == 0.0 and not np.signbit(z[0])
    # decay 0 copies p (omd = 1: e + (p - e), exact when p - e is)
    assert ema_update_ref(np.array([3.0], np.float32), np.array([1.0], np.float32), 0.0)[0] == 3.0
    # inputs are not modified
    e = np.ones(4, np.float32); q = np.full(4, 2.0, np.float32)
    ema_update_ref(q, e, 0.5)
    assert np.all(e == 1.0) and np.all(q == 2.0)
    assert np.all(ema_update_ref(q, e, 0.5) == 1.5)


def test_cli_flags(monkeypatch, capsys):
    import histopathology_gan as H
    base = ["histopathology_gan.py", "--config", "c.json"]
    monkeypatch.setattr(sys, "argv", base)
    a = H.parse_args()
    assert a.g_ema == 0.0 and a.g_ema_warmup == 1
    monkeypatch.setattr(sys, "argv", base + ["--g_ema", "0.999", "--g_ema_warmup", "0"])
    a = H.parse_args()
    assert a.g_ema == 0.999 and a.g_ema_warmup == 0
    for bad in (["--g_ema", "1.0"], ["--g_ema", "-0.1"], ["--g_ema", "nan"], ["--g_ema", "1.5"], ["--g_ema_warmup", "2"]):
        monkeypatch.setattr(sys, "argv", base + bad)
        with pytest.raises(SystemExit) as ex:
            H.parse_args()
        assert ex.value.code != 0
        assert "--g_ema" in capsys.readouterr().err


def test_param_ema_rejects_a_bad_decay_and_a_foreign_module():
    from rna_gan_amd.ema import ParamEMA
    import rna_gan_amd as P
    assert P.ParamEMA is ParamEMA
    G = P.DCGANGenerator(16, 16, 3, 4)
    for bad in (1.0, -0.1, 1.5, float("nan")):
        with pytest.raises(ValueError):
            ParamEMA(G, decay=bad)
    with pytest.raises(TypeError):
        ParamEMA(nn.Linear(2, 2))
    ema = ParamEMA(G, decay=0.5, warmup=False)
    twin = ema.module
    assert type(twin) is type(G) and not twin.training and not any(p.requires_grad for p in twin.parameters())
    sd, st = G.state_dict(), twin.state_dict()
    assert list(sd.keys()) == list(st.keys())
    mine = {t.untyped_storage().data_ptr() for t in sd.values()}
    for k in sd:
        assert sd[k].shape == st[k].shape and torch.equal(sd[k], st[k])
        assert st[k].untyped_storage().data_ptr() not in mine
    assert G.training and all(p.requires_grad for p in G.parameters())       # the live module is left as it was
    # an optimizer bound to another module refuses the average
    other = P.DCGANGenerator(16, 16, 3, 4)
    opt = P.Adam(other.parameters(), lr=1e-4).bind(other)
    with pytest.raises(ValueError):
        opt.attach_ema(ema)
