#!/usr/bin/env python
"""
Generate tests/golden/mcts_tables.npz by IMPORTING the reference's MCTS (planning/mcts_zero/mcts.py) and running its own
compute_uct (:280-296, force_playouts True and False), normalize_q_values (:267-278) and get_policy (:83-143, with
num_mcts_simulations = 0: the read-out alone) on the node rows of tests/mcts_table_cases.py, expanded to the dense arrays over all
actions that the reference keeps (Nsa, Qsa, Ps, Vs: zeros / False outside the valid set).

    python tests/golden/gen_mcts_tables_golden.py REFERENCE_CHECKOUT [--check]      (or IPP_REFERENCE=REFERENCE_CHECKOUT)

The fixture holds numbers only (recorded results and the digests of the inputs they were recorded from):
    sel/{case}/{node}/uct0, uct1   compute_uct(force_playouts=False / True) of an expanded node of a select case, [A], -inf outside
    sel/{case}/{node}/qn           normalize_q_values(Qsa), [A]
    ro/{case}/{root}/kept          the action index get_policy's np.random.choice kept among the most visited (seeded), -1: none of
                                   the valid ones (every action unvisited: the reference draws among ALL actions)
    ro/{case}/{root}/tie_u         the uniform that makes the same choice among the valid ties: (rank + 0.5) / ties
    ro/{case}/{root}/T{t}d{d}      the policy [A] at temperature t and deploy_time d; a 0-length array where get_policy returned None
    digest/{case}                  sha256 of the case's tables (tests/test_mcts_tables_host.py: the fixture belongs to the cases)
Temperature 0 is not recorded: the device read-out refuses it.  The archive is written with fixed time stamps, so that running the
generator again gives the same bytes; --check compares a new recording with the committed file instead of writing it.
"""
import hashlib
import io
import os
import sys
import types
import zipfile
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
PATH = os.path.join(ROOT, "tests", "golden", "mcts_tables.npz")
SCORE_CASES = ("kmax-64", "kmax-65", "kmax-130", "kmax-257", "forced-ties", "tie-break-random", "budget-horizon", "transposition")
DEPLOY_TEMPERATURES = (1.0, 0.5)


def digest(st):
    """sha256 over a case's tables and scalars."""
    h = hashlib.sha256()
    for k in sorted(st):
        v = st[k]
        h.update(k.encode())
        h.update(np.ascontiguousarray(v).tobytes() if isinstance(v, np.ndarray) else repr(v).encode())
    return np.frombuffer(h.digest(), dtype=np.uint8).copy()


def dense_node(st, node):
    """(Nsa, Qsa, Ps, Vs, Ns) of a node the way the reference keeps them."""
    A, K = st["num_actions"], int(st["n_k"][node])
    idx = st["t_idx"][node, :K]
    out = []
    for k in ("t_nsa", "t_qsa", "t_ps"):
        a = np.zeros(A)
        a[idx] = st[k][node, :K]
        out.append(a)
    vs = np.zeros(A, dtype=bool)
    vs[idx] = True
    return out[0], out[1], out[2], vs, float(st["n_ns"][node])


def reference_mcts(ref_mcts, st, sims=0):
    """An MCTS object with the attributes compute_uct, normalize_q_values and get_policy read, no mapping and no queues behind it."""
    m = ref_mcts.MCTS.__new__(ref_mcts.MCTS)
    m.hyper_params = {"forced_playout_factor": st["fpf"], "max_valid_action_distance": 11.5}
    m.puct_init, m.puct_base, m.num_simulations = st["puct_init"], st["puct_base"], sims
    m.actions_np = st["actions"]
    m.Qsa, m.Nsa, m.Ns, m.Vs, m.Ps = {}, {}, {}, {}, {}
    return m


def record(ref):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, ref)
    sys.dont_write_bytecode = True
    for name in ("cv2", "imageio"):  # (imported at module level by the reference's simulations and sensors; not used here)
        if name not in sys.modules:
            try:
                __import__(name)
            except ImportError:
                sys.modules[name] = types.ModuleType(name)
    import planning.mcts_zero.mcts as ref_mcts

    from tests import mcts_table_cases as mc

    out = {}
    for case in SCORE_CASES:
        st = mc.SELECT_CASES[case]()["st"]
        out[f"digest/sel/{case}"] = digest(st)
        m = reference_mcts(ref_mcts, st)
        for node in np.nonzero(st["n_flags"] & mc.EXPANDED)[0]:
            m.Nsa[0], m.Qsa[0], m.Ps[0], m.Vs[0], m.Ns[0] = dense_node(st, node)
            with np.errstate(all="ignore"):
                out[f"sel/{case}/{node}/uct0"] = m.compute_uct(0, force_playouts=False)
                out[f"sel/{case}/{node}/uct1"] = m.compute_uct(0, force_playouts=True)
                out[f"sel/{case}/{node}/qn"] = np.array(ref_mcts.MCTS.normalize_q_values(m.Qsa[0].copy()))
    for ci, case in enumerate(mc.READOUT_CASES):
        st = mc.READOUT_CASES[case]()["st"]
        out[f"digest/ro/{case}"] = digest(st)
        for j in range(st["roots"]):
            node = j * st["nodes_per_root"]
            if not st["n_flags"][node] & mc.EXPANDED:
                continue  # (the reference has no row for such a root)
            nsa, qsa, ps, vs, ns = dense_node(st, node)
            root = ref_mcts.Node(np.array([ci, j]))
            rep = root.state_representation()
            seed = 7000 + 31 * ci + j
            np.random.seed(seed)
            kept = int(np.random.choice((nsa == np.max(nsa)).nonzero()[0]))
            ties = np.nonzero(nsa[vs] == np.max(nsa))[0] if vs.any() else np.zeros(0, int)
            valid_pos = np.cumsum(vs) - 1
            if vs.any() and vs[kept] and (np.max(nsa) > 0 or vs.all()):
                out[f"ro/{case}/{j}/kept"] = np.array(kept)
                out[f"ro/{case}/{j}/tie_u"] = np.array((int(np.nonzero(ties == valid_pos[kept])[0][0]) + 0.5) / len(ties))
            else:
                out[f"ro/{case}/{j}/kept"] = np.array(-1)
                out[f"ro/{case}/{j}/tie_u"] = np.array(0.0)
            for t, d, _ in mc.readout_modes(case):
                m = reference_mcts(ref_mcts, st)
                m.Nsa[rep], m.Qsa[rep], m.Ps[rep], m.Vs[rep], m.Ns[rep] = nsa.copy(), qsa.copy(), ps.copy(), vs.copy(), ns
                np.random.seed(seed)
                with np.errstate(all="ignore"):
                    res = m.get_policy(root, 0, np.array([2.0, 2.0, 14.0]), 50.0, None, temperature=t, deploy_time=bool(d))
                out[f"ro/{case}/{j}/T{t}d{d}"] = np.zeros(0) if res is None else np.array(res[0], dtype=np.float64)
    return out


def write_archive(path, arrays):
    """An .npz with fixed time stamps: the same arrays give the same bytes."""
    with zipfile.ZipFile(path, "w") as z:
        for k in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asarray(arrays[k]), allow_pickle=False)
            info = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue(), compress_type=zipfile.ZIP_DEFLATED, compresslevel=zlib.Z_BEST_COMPRESSION)


def main():
    args = [a for a in sys.argv[1:] if a != "--check"]
    ref = args[0] if args else os.environ.get("IPP_REFERENCE")
    if not ref or not os.path.isdir(ref):
        sys.exit("usage: gen_mcts_tables_golden.py REFERENCE_CHECKOUT [--check] (the fixture can only be recorded next to the reference)")
    out = record(ref)
    if "--check" in sys.argv[1:]:
        old = np.load(PATH)
        assert sorted(old.files) == sorted(out), "the committed fixture holds other arrays"
        for k in out:
            a, b = np.asarray(out[k]), old[k]
            assert a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes(), k
        print(f"{PATH}: {len(out)} arrays reproduced bit for bit")
        return
    write_archive(PATH, out)
    print(f"wrote {PATH}: {len(out)} arrays, {os.path.getsize(PATH)} bytes")


if __name__ == "__main__":
    main()
