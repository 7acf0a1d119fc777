"""CPU: the host policy of the dynamic loss scale (sky_embeddings_amd.loss_scale.LossScaler) against torch's own
``torch._amp_update_scale_`` -- what ``torch.amp.GradScaler.update()`` runs -- step by step, and the scaler's argument checks and
checkpoint round trip.  (The exported surface -- skyemb_grad_probe / skyemb_adamw_guarded in the header and in _lib.PROTOTYPES --
is held by tests/test_abi_cpu.py.)"""
import pytest
import torch

from sky_embeddings_amd import _lib
from sky_embeddings_amd.loss_scale import LossScaler, is_power_of_two, make_loss_scaler

# consecutive overflows, overflows with the tracker at 1 and at 2 of 3, growth twice in a row, an overflow right after a growth
FLAGS = [0, 0, 0, 1, 1, 0, 1, 0, 0, 1, 0, 0, 0, 0, 0, 0, 1, 1, 1, 0, 0, 0, 1]


def torch_sequence(init, growth, backoff, interval, flags):
    scale, tracker = torch.full((1,), init, dtype=torch.float32), torch.zeros(1, dtype=torch.int32)
    out = []
    for f in flags:
        torch._amp_update_scale_(scale, tracker, torch.full((1,), float(f)), growth, backoff, interval)
        out.append((float(scale), int(tracker)))
    return out


@pytest.mark.parametrize("init,growth,backoff", [(2.0 ** 16, 2.0, 0.5), (2.0 ** 4, 4.0, 0.25), (1.0, 2.0, 0.125)])
def test_update_matches_torch_amp_update_scale(init, growth, backoff):
    want = torch_sequence(init, growth, backoff, 3, FLAGS)
    sc = LossScaler(init_scale=init, growth_factor=growth, backoff_factor=backoff, growth_interval=3)
    skipped = 0
    for k, f in enumerate(FLAGS):
        sc.update(bool(f))
        skipped += f
        assert (sc.scale, sc.growth_tracker) == want[k], (k, f, sc.scale, sc.growth_tracker, want[k])
        assert sc.skipped_steps == skipped and sc.last_overflow == bool(f)
    assert len({s for s, _ in want}) > 3          # the script really moves the scale both ways


def test_growth_stops_where_fp32_ends():
    want = torch_sequence(2.0 ** 126, 2.0, 0.5, 1, [0, 0, 0, 1])
    sc = LossScaler(init_scale=2.0 ** 126, growth_interval=1)
    for k, f in enumerate([0, 0, 0, 1]):
        sc.update(bool(f))
        assert (sc.scale, sc.growth_tracker) == want[k]
    assert want[1][0] == want[2][0] == 2.0 ** 127


def test_fixed_scale_counts_skips_but_never_moves():
    sc = LossScaler(init_scale=2.0 ** 10, growth_interval=2, dynamic=False)
    for f in (0, 0, 0, 1, 1, 0, 0, 0):
        sc.update(bool(f))
        assert sc.scale == 2.0 ** 10 and sc.growth_tracker == 0
    assert sc.skipped_steps == 2
    fixed = make_loss_scaler(2 ** 10)
    assert not fixed.dynamic and fixed.scale == 1024.0
    assert make_loss_scaler("2**10").scale == 1024.0 and make_loss_scaler("1024").scale == 1024.0 and not make_loss_scaler("4.0").dynamic
    dyn = make_loss_scaler("dynamic")
    assert dyn.dynamic and dyn.scale == 2.0 ** 16 and dyn.growth_interval == 2000 and (dyn.growth_factor, dyn.backoff_factor) == (2.0, 0.5)
    assert make_loss_scaler(sc) is sc


def test_powers_of_two_only():
    assert all(is_power_of_two(v) for v in (1, 2.0, 0.5, 2.0 ** -20, 2.0 ** 100, 65536))
    assert not any(is_power_of_two(v) for v in (0, -2.0, 3, 0.3, 65535.0, float("inf"), float("nan"), "x", None))
    for kw in (dict(init_scale=3.0), dict(init_scale=0.0), dict(init_scale=-4.0), dict(growth_factor=3.0), dict(growth_factor=1.0),
               dict(growth_factor=0.5), dict(backoff_factor=0.3), dict(backoff_factor=1.0), dict(backoff_factor=2.0),
               dict(growth_interval=0)):
        with pytest.raises(AssertionError):
            LossScaler(**kw)
    for spec in (3, 1000.0, "1000", "sometimes", "2**0.5", 0, "__import__('os')"):
        with pytest.raises(ValueError):
            make_loss_scaler(spec)
    with pytest.raises(AssertionError):
        LossScaler().load_state_dict({"scale": 3.0, "growth_tracker": 0, "skipped_steps": 0})


def test_state_dict_round_trip_continues_the_sequence():
    a = LossScaler(growth_interval=3)
    for f in FLAGS[:8]:
        a.update(bool(f))
    sd = a.state_dict()
    assert sorted(sd) == ["growth_tracker", "scale", "skipped_steps"]
    assert sd == {"scale": a.scale, "growth_tracker": a.growth_tracker, "skipped_steps": 3} and a.growth_tracker == 1
    b = LossScaler(growth_interval=3)
    b.load_state_dict(sd)
    for f in FLAGS[8:]:
        a.update(bool(f))
        b.update(bool(f))
        assert (a.scale, a.growth_tracker, a.skipped_steps) == (b.scale, b.growth_tracker, b.skipped_steps)


def test_bindings_cover_the_guard_entry_points():
    probe, guarded, plain = (_lib.PROTOTYPES[k][1] for k in ("skyemb_grad_probe", "skyemb_adamw_guarded", "skyemb_adamw"))
    assert len(probe) == 5
    # skyemb_adamw's list with the skip word in front of the stream
    assert guarded[:-2] == plain[:-1] and guarded[-2:] == [_lib.c_vp, _lib.c_vp]
