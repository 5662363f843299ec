#!/usr/bin/env python
"""
Generate tests/golden/per.npz by IMPORTING the reference's PrioritizedExperienceReplayBuffer (planning/mcts_zero/replay_buffers.py:
104-141) and recording what it does over six training iterations of sample -> update(indices, losses + 1e-8) -> step.

    python tests/golden/gen_per_golden.py REFERENCE_CHECKOUT          (or IPP_REFERENCE=REFERENCE_CHECKOUT)

The fixture holds numbers only (inputs and recorded results, some tens of KB): per case c, one row per iteration,
    c{c}_u           the uniforms np.random.choice consumed (re-derived from the iteration's seed with np.random.random_sample(n))
    c{c}_indices     sample_indices
    c{c}_weights     the float32 importance-sampling weights
    c{c}_beta        beta at the sample; c{c}_beta_next after step()
    c{c}_values      the made-up losses + 1e-8 handed to update()
    c{c}_priorities  the priorities after the update
and c{c}_meta = (L, batch, alpha, beta0, num_epochs, total_steps).  torchvision is stubbed when it is absent (the module imports
it for the uniform buffer's augmentation only); the train-data directory is a temporary directory of tiny dummy samples.
"""
import bz2
import os
import pickle
import sys
import tempfile
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
CASES = [(L, batch, 0.75, beta0, 3) for (L, batch) in ((7, 4), (64, 32), (300, 32)) for beta0 in (0.4, 0.5)]
ITERATIONS = 6


def main():
    ref = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("IPP_REFERENCE")
    if not ref or not os.path.isdir(ref):
        sys.exit("usage: gen_per_golden.py REFERENCE_CHECKOUT (the fixture can only be generated next to the reference)")
    sys.path.insert(0, ref)
    try:
        import torchvision  # noqa: F401
    except ImportError:
        sys.modules["torchvision"] = types.ModuleType("torchvision")
    from planning.mcts_zero import replay_buffers as rb

    out = {}
    repeats = 0
    with tempfile.TemporaryDirectory() as tmp:
        for c, (L, batch, alpha, beta0, epochs) in enumerate(CASES):
            rb.TRAIN_DATA_DIR = os.path.join(tmp, f"case{c}")
            os.makedirs(os.path.join(rb.TRAIN_DATA_DIR, "iter_0"))
            for i in range(L):  # (input_feature_planes, policy, value, reward, valid_actions_msk)
                with bz2.BZ2File(os.path.join(rb.TRAIN_DATA_DIR, "iter_0", f"sample_{i:04d}.pkl.bz2"), "wb") as f:
                    pickle.dump((np.full((1, 2, 2), float(i)), np.array([1.0, 0.0]), float(i), 0.0, np.array([1, 0])), f)
            buf = rb.PrioritizedExperienceReplayBuffer(0, 1, batch_size=batch, alpha=alpha, beta0=beta0, num_epochs=epochs)
            assert len(buf) == L and buf.sample_size == batch
            out[f"c{c}_meta"] = np.array([L, batch, alpha, beta0, epochs, buf.total_steps], dtype=np.float64)
            losses = np.random.RandomState(1000 + c)  # (made-up losses: not the global stream the buffer draws from)
            rec = {k: [] for k in ("u", "indices", "weights", "beta", "beta_next", "values", "priorities")}
            for t in range(ITERATIONS):
                seed = 100 * c + t
                np.random.seed(seed)
                u = np.random.random_sample(batch)
                np.random.seed(seed)
                beta = float(buf.beta)
                *_, idx, w = buf.sample()
                assert w.dtype == np.float32
                values = losses.gamma(2.0, 0.5, size=batch) + 1e-8
                buf.update(idx, values)
                buf.step()
                repeats += len(idx) - len(np.unique(idx))
                for k, v in zip(rec, (u, np.asarray(idx, dtype=np.int64), w, beta, float(buf.beta), values, buf.priorities.copy())):
                    rec[k].append(v)
            for k, v in rec.items():
                out[f"c{c}_{k}"] = np.array(v)
    assert repeats > 0, "no recorded minibatch repeats an index: the last-occurrence-wins update would go unchecked"
    path = os.path.join(ROOT, "tests", "golden", "per.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {len(out)} arrays, {os.path.getsize(path)} bytes, {repeats} repeated indices")


if __name__ == "__main__":
    main()
