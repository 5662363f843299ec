"""
GPU tests of the compact replay ring's persistence (ReplayBuffer.state_dict / load_state_dict, SelfPlay.state_dict / load_state_dict;
the archived episodes travel as packed slot records: IPPEngine.export_slots / import_slots, csrc/k_slots.h) on the SelfPlay
configuration of tests/test_hip_replay_compact.py (B = 3, history 2, 5-step budget episodes, 8 sequential simulations, no network), with
the default E = S and with E = 2 (archive slots reused, rows evicted), after a run long enough that the ring has wrapped:
  * a state dict that went through torch.save / torch.load(map_location="cpu") restores, in a fresh SelfPlay of the same arguments, a
    ring with the same committed rows, the same gathered outputs and the same minibatches at the same draw count, bit for bit;
  * no PENDING row survives; the restored loop plays on and its new rows have finite planes;
  * another B, E or slot count, and a dense-planes ring, are refused.
"""
import numpy as np
import pytest

from tests.test_hip_replay_compact import bits_equal, host, make, same_batch

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(600)]

B = 3


def through_disk(sd, path):
    import torch

    torch.save(sd, path)
    return torch.load(path, map_location="cpu")


@pytest.mark.parametrize("E", [None, 2])
def test_a_saved_ring_restores_bit_for_bit(tmp_path, E):
    import torch

    from ipp_rl_amd.planning.mcts_zero.selfplay import COMMITTED, PENDING, archive_slots_in_use

    kw = dict(archive_episodes=E) if E else {}
    if E:
        kw["initial_budget"] = 7.0  # (one- and two-step episodes: the archive slots are reused while the rows are still in the ring)
    one = make("compact", B, seed=6, **kw)
    S = one.slots
    t = 0
    r = one.replay
    # (until the ring has wrapped, every env has reused an archive place with E = 2, and some episode is running: its rows are pending)
    while t < 2 * S + 2 or int(r.episodes.min().item()) <= (E or 1) or int((r.flags == PENDING).sum().item()) == 0:
        one.step()
        t += 1
        assert t < 8 * S
    assert (r.evicted > 0) == bool(E) and len(r) > 0
    sd = one.state_dict()
    used = archive_slots_in_use(host(r.episodes), B, r.archive_episodes)
    assert host(sd["archive_slots"]).tolist() == used.tolist() and sd["archive"]["what"] == 1 and len(used) > 0
    assert int(sd["archive"]["offsets"].numel()) == len(used) + 1 and sd["archive"]["blob"].is_cuda
    assert sd["draws"] == r.draws and sd["step"] == one.t == t
    assert sd["geometry"] == dict(slots=S, num_envs=B, kmax=r.kmax, num_actions=r.num_actions, side=r.side, history=2, E=r.archive_episodes,
                                  compact=True)
    loaded = through_disk(sd, tmp_path / "ring.pt")
    assert not loaded["flags"].is_cuda and not loaded["archive"]["blob"].is_cuda
    two = make("compact", B, seed=6, **kw)
    two.load_state_dict(loaded)
    q = two.replay
    assert len(q) == len(r) and q.evicted == r.evicted and q.draws == r.draws and two.t == one.t
    rows = r.committed_rows()
    assert torch.equal(q.committed_rows(), rows) and rows.numel() > 0
    assert int((q.flags == PENDING).sum().item()) == 0
    assert torch.equal(q.flags == COMMITTED, r.flags == COMMITTED)
    for name in ("episodes", "last_rank", "episode_tag", "iter"):
        assert torch.equal(getattr(q, name), getattr(r, name)), name
    for x, y in zip(r.gather_rows(rows), q.gather_rows(rows)):
        assert bits_equal(x, y)
    x, y = r.sample(8, num_augmented_samples=1), q.sample(8, num_augmented_samples=1)
    same_batch(x, y)
    assert torch.isfinite(y[0]).all() and bits_equal(r.last_offsets, q.last_offsets)
    same_batch(r.prioritized(batch_size=4).sample(), q.prioritized(batch_size=4).sample())
    assert q.draws == r.draws == sd["draws"] + 2
    # the restored loop plays on: its ring position is the saved one, every committed row has planes
    two.run(S)
    assert two.t == t + S and len(q) > 0
    planes = q.gather_rows(q.committed_rows())[0]
    assert torch.isfinite(planes).all()
    one.close()
    two.close()


def test_other_geometries_and_dense_rings_are_refused():
    one = make("compact", B, seed=6)
    for _ in range(one.slots):
        one.step()
    sd = one.state_dict()
    for kw, field in ((dict(B=B + 1), "num_envs"), (dict(archive_episodes=2), "E"), (dict(capacity=B * (one.slots + 1)), "slots")):
        other = make("compact", kw.pop("B", B), seed=6, **kw)
        with pytest.raises(ValueError, match=f"{field} = "):
            other.load_state_dict(sd)
        other.close()
    bare = make(False, B, seed=6)
    with pytest.raises(ValueError, match="history = 2"):
        bare.load_state_dict(sd)
    for _ in range(one.slots):
        bare.step()
    again = make(False, B, seed=6)
    again.load_state_dict(bare.state_dict())  # (a ring without planes has nothing but its row arrays)
    assert bits_equal(again.replay.value, bare.replay.value) and len(again.replay) == len(bare.replay) and "archive" not in bare.state_dict()
    dense = make(True, B, seed=6)
    with pytest.raises(ValueError, match="GiB"):
        dense.state_dict()
    with pytest.raises(ValueError, match="dense-planes"):
        dense.load_state_dict(sd)
    for s in (one, bare, again, dense):
        s.close()
