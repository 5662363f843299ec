"""
Host side of the policy-value network (planning/mcts_zero/networks.py), against tests/golden/pvnet.npz and pvnet_edges.npz recorded from
the reference's PolicyValueNetwork (tests/golden/gen_pvnet_golden.py).  d32 = max |ref32 - ref64| per configuration and output is the reference's own
fp32 rounding distance, the unit of the bounds:
  * the restated module takes the reference's state_dict with strict=True and reproduces ref32 within 4 d32 (the same arithmetic in
    the same framework; the factor covers another conv algorithm);
  * run_plan_numpy in fp64 on the folded plan reproduces ref64 and the recorded block outputs to 1e-9 relative: folding is exact
    algebra, and fp64 leaves that much room at these depths;
  * the edges of the device kernels that d, e, f and g exist for are facts about their plans, asserted here from the kernels' own
    tile constants, and the condition under which their seeds were kept holds on the fixture's own arrays;
  * shared weights are packed once and the op count is the one the block schedule implies;
  * every ValueError of the plan and of DevicePolicyValueNet fires before the device is touched.
No GPU.
"""
import numpy as np
import pytest
import torch

from tests import pvnet_cases as pc

NAMES = ("a", "b", "c", "d", "e", "f", "g")


def _module(case):
    from ipp_rl_amd.planning.mcts_zero.networks import PolicyValueNetwork

    net = PolicyValueNetwork(case["hp"], case["md"]).eval()
    net.load_state_dict(case["state_dict"], strict=True)
    return net


def _predict(net, planes, idx, dtype):
    n, A = planes.shape[0], net.num_actions
    mask = np.zeros((n, A))
    for r in range(n):
        mask[r, idx[r][idx[r] >= 0]] = 1.0
    with torch.no_grad():
        lp, v, reward, dec = net.to(dtype)(torch.from_numpy(planes).to(dtype), torch.from_numpy(mask).to(dtype))
    assert reward is None and dec is None and lp.shape == (n, A) and v.shape == (n, 1)
    pol = torch.exp(lp).double().numpy()
    prior = np.zeros(idx.shape)
    for r in range(n):
        ids = idx[r][idx[r] >= 0]
        prior[r, :len(ids)] = pol[r, ids]
    v = v.double().numpy().reshape(n)
    return prior, v * v + 2 * v


@pytest.mark.parametrize("name", NAMES)
def test_module_takes_the_reference_state_dict_and_reproduces_ref32(name):
    case = pc.case(name)
    net = _module(case)  # strict=True
    assert list(net.state_dict().keys()) == case["keys"]
    prior, value = _predict(net, case["planes"], case["valid_idx"], torch.float32)
    e_p, e_v = np.abs(prior - case["prior32"]).max(), np.abs(value - case["value32"]).max()
    print(f"{name}: |module - ref32| prior {e_p:.3g} ({e_p / case['d32_prior']:.2f} d32) value {e_v:.3g} ({e_v / case['d32_value']:.2f} d32)")
    assert e_p <= 4 * case["d32_prior"] and e_v <= 4 * case["d32_value"]


def test_module_details():
    """The details that are easy to lose."""
    from ipp_rl_amd.planning.mcts_zero.networks import STRIDE2_BLOCKS, encoder_block_kind

    net = _module(pc.case("a"))
    sep = net.encoder.separable_residual_block_s1
    assert sep.bn1.eps == sep.bn2.eps == 1e-3
    assert net.encoder.down_sample_block[0][1].eps == net.encoder.mix_global_context_s1.bn_layer.eps == sep.down_sample_layer[1].eps == 1e-5
    assert STRIDE2_BLOCKS == (0, 1, 3, 5)
    assert [encoder_block_kind(i, True, True).startswith("mix") for i in range(10)] == [i > 0 and i % 3 == 0 for i in range(10)]
    assert encoder_block_kind(3, True, True) == "mix_global_context_s2" and encoder_block_kind(6, False, True) == "mix_global_context_s1"
    assert encoder_block_kind(3, False, False) == "residual_block_s2" and encoder_block_kind(2, True, False) == "separable_residual_block_s1"
    assert isinstance(net.value_head.head[2], torch.nn.Softplus) and len(net.value_head.head) == 3


@pytest.mark.parametrize("name", NAMES)
def test_plan_in_fp64_reproduces_ref64(name):
    from ipp_rl_amd.planning.mcts_zero.networks import build_plan, check_plan, run_plan_numpy

    case = pc.case(name)
    plan, w = build_plan(case["hp"], case["md"], case["state_dict"], case["cfg"]["side"], dtype=np.float64)
    check_plan(plan, w.size)
    prior, value = run_plan_numpy(plan, w, case["planes"], case["valid_idx"], dtype=np.float64)
    e_p = np.abs(prior - case["prior64"]).max() / np.abs(case["prior64"]).max()
    e_v = np.abs(value / case["value64"] - 1).max()
    print(f"{name}: plan(fp64) vs ref64: prior {e_p:.3g} value {e_v:.3g} (relative)")
    assert e_p <= 1e-9 and e_v <= 1e-9
    K = (case["valid_idx"] >= 0).sum(axis=1)
    assert np.all(prior[K == 0] == 0) and np.all(prior[case["valid_idx"] < 0] == 0)


def test_plan_taps_reproduce_the_block_outputs():
    from ipp_rl_amd.planning.mcts_zero.networks import build_plan, run_plan_numpy

    with_taps = [n for n in NAMES if pc.recorded_taps(n)]
    assert with_taps == ["a", "d", "e", "f", "g"]
    for cfg in with_taps:
        case = pc.case(cfg)
        plan, w = build_plan(case["hp"], case["md"], case["state_dict"], case["cfg"]["side"], dtype=np.float64)
        rows = list(case["tap_rows"])
        assert [b for b, _ in plan.blocks] == pc.block_names(cfg) and len(case["taps64"]) == len(case["tap_names"]) > 0
        if cfg in ("a", "d"):
            assert [b for b, _ in plan.blocks] == case["tap_names"]
        for name, want in zip(case["tap_names"], case["taps64"]):
            _, _, tap = run_plan_numpy(plan, w, case["planes"][rows], case["valid_idx"][rows], dtype=np.float64, tap_op=plan.tap(name))
            assert tap.shape == want.shape, (cfg, name)
            assert np.abs(tap - want).max() <= 1e-9 * np.abs(want).max(), (cfg, name)


def _schedule(name):
    """(op count, packed floats) the block schedule implies, counted from the configuration alone."""
    from ipp_rl_amd.planning.mcts_zero.networks import encoder_block_kind

    c = pc.CONFIGS[name]
    C, G, A = c["channels"], c["pooled"], c["side"] ** 2 * c["levels"]
    conv = lambda ci, kh, kw: C * ci * kh * kw + C  # noqa: E731  (weights + the folded bias)
    mix_w = lambda stride: 2 * conv(C, 3, 3) + 2 * G + (C - G) * 2 * G + (C - G) + (conv(C, 1, 1) if stride == 2 else 0)  # noqa: E731
    ops_of = {"residual_block_s1": 3, "residual_block_s2": 3, "separable_residual_block_s1": 5, "separable_residual_block_s2": 6,
              "mix_global_context_s1": 3, "mix_global_context_s2": 4}
    floats_of = {"residual_block_s1": conv(C, 1, 1) + 2 * conv(C, 3, 3), "residual_block_s2": conv(C, 1, 1) + 2 * conv(C, 3, 3),
                 "separable_residual_block_s1": conv(C, 1, 1) + 4 * conv(C, 3, 1), "separable_residual_block_s2": 2 * conv(C, 1, 1) + 4 * conv(C, 3, 1),
                 "mix_global_context_s1": mix_w(1), "mix_global_context_s2": mix_w(2)}
    kinds = [encoder_block_kind(i, c["separable"], c["mixing"]) for i in range(c["blocks"])]
    ops, floats = 1 + sum(ops_of[k] for k in kinds), conv(c["input_channels"], 7, 7) + sum(floats_of[k] for k in set(kinds))
    for blocks in c["heads"]:
        mixed = c["mixing"] and blocks > 0
        ops += (3 if mixed else 0) + (blocks - (1 if mixed else 0)) + 1  # trunk + pool
        floats += (mix_w(1) if mixed else 0) + (conv(C, 3, 3) if blocks > (1 if mixed else 0) else 0)
    return ops + 2, floats + 2 * C + 1 + A * 2 * C + A, kinds


@pytest.mark.parametrize("name", NAMES)
def test_plan_packs_shared_weights_once(name):
    from ipp_rl_amd.planning.mcts_zero.networks import PV_CONV, build_plan

    case = pc.case(name)
    plan, w = build_plan(case["hp"], case["md"], case["state_dict"], case["cfg"]["side"])
    n_ops, n_floats, kinds = _schedule(name)
    assert len(plan.ops) == n_ops == {"a": 63, "b": 20, "c": 47, "d": 30, "e": 34, "f": 25, "g": 13}[name]
    assert w.dtype == np.float32 and w.size == plan.n_floats == n_floats
    spans = sorted(plan.packed.values())
    assert spans[0][0] == 0 and all(a[0] + a[1] == b[0] for a, b in zip(spans, spans[1:])) and spans[-1][0] + spans[-1][1] == w.size
    # a block that runs k times contributes its ops k times and its weights once
    convs = [op for op in plan.ops if op["kind"] == PV_CONV]
    repeats = max(kinds.count(k) for k in set(kinds))
    assert repeats > 1
    offs = [op["w_off"] for op in convs]
    assert max(offs.count(o) for o in set(offs)) == max(repeats, max(case["cfg"]["heads"]) - (1 if case["cfg"]["mixing"] else 0))
    # nothing the forward never runs is packed
    assert not any(k.startswith("decoder") for k in plan.packed)
    if case["cfg"]["separable"]:
        assert not any(".residual_block_s" in k for k in plan.packed)


def _kernel_constants():
    """kBM, kBN, kBK, kThreads as csrc/k_pvnet.h states them."""
    import os
    import re

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    txt = open(os.path.join(root, "ipp-rl_amd", "csrc", "k_pvnet.h")).read()
    line = re.search(r"constexpr int (kBM = \d+, kBN = \d+, kBK = \d+, kThreads = \d+);", txt).group(1)
    return {k: int(v) for k, v in (item.split(" = ") for item in line.split(", "))}


def test_edge_configurations_reach_their_edges():
    """What d, e, f and g are for, as facts about their plans and the kernels' tile constants: a later change of kBM / kBN / kBK /
    kThreads or of a configuration cannot silently un-cover an edge ("Policy-value network", lists them)."""
    from ipp_rl_amd.planning.mcts_zero.networks import PV_CONV, PV_MIX, PV_POOL, build_plan

    k = _kernel_constants()
    kBN, kBK, T, mfma_n = k["kBN"], k["kBK"], k["kThreads"], 16
    assert (k["kBM"], kBN, kBK, T) == (64, 64, 32, 256)
    ops = {}
    for name in pc.EDGE_NAMES:
        case = pc.case(name)
        plan, _ = build_plan(case["hp"], case["md"], case["state_dict"], case["cfg"]["side"])
        ops[name] = plan.ops
    convs = {n: [op for op in ops[n] if op["kind"] == PV_CONV] for n in ops}
    pools = {n: [op for op in ops[n] if op["kind"] == PV_POOL] for n in ops}
    mixes = {n: [op for op in ops[n] if op["kind"] == PV_MIX] for n in ops}
    conv_k = {n: sorted({op["kh"] * op["kw"] * op["cin"] for op in convs[n]}) for n in ops}
    for name in pc.EDGE_NAMES:  # more than one output-channel tile in every conv
        assert all(op["cout"] > kBN for op in convs[name]), name
    for name in ("d", "g"):  # the last tile ends inside a 16-column MFMA block
        assert all(op["cout"] % mfma_n != 0 for op in convs[name]), name
    assert [-(-op["cout"] // kBN) for op in convs["d"][:1] + convs["e"][:1] + convs["f"][:1] + convs["g"][:1]] == [2, 2, 5, 3]
    # e, as shipped: no K tail in any conv between activations; its stem alone (7 x 7 x 16 planes = 784 = 24.5 chunks) has one
    stem_k = 49 * pc.CONFIGS["e"]["input_channels"]
    assert convs["e"][0]["src"] == -1 and conv_k["e"] == sorted({stem_k, 128, 384, 1152}) and all(K % kBK == 0 for K in conv_k["e"] if K != stem_k)
    assert not any(K % kBK == 0 for K in conv_k["d"]) and {648, 216, 72} <= set(conv_k["d"])
    # pool_channels: the g0 loop twice (f), one slice with idle threads (g), pixel slices with idle threads (d's mix: T // 24 = 10, 16 idle)
    assert any(op["cin"] >= T for op in pools["f"]) and all(T // 2 < op["cin"] < T for op in pools["g"])
    assert any(op["cout"] - op["cin"] > T for op in mixes["f"])  # the context loop of k_pv_mix twice
    assert all(op["cin"] == 24 and T % op["cin"] != 0 for op in mixes["d"]) and mixes["d"] and not mixes["g"]
    # the head pools average more than one pixel, against the reference
    assert all(op["hin"] * op["win"] == 9 for op in pools["d"]) and all(op["hin"] * op["win"] == 4 for op in pools["e"] + pools["g"])
    for name in pc.EDGE_NAMES:  # a second pass of the policy head's loops over the slots
        K = (pc.case(name)["valid_idx"] >= 0).sum(axis=1)
        assert pc.case(name)["kmax"] == 300 > T and K[0] == 1 and K[1] == 300 and K[2] == 0 and np.all(K[3:] > T), name
    # the value head's dot product over 2 C pooled values takes a second pass in f and g; f's value head is clamped by its ReLU on
    # every row (value = softplus(0)^2 + 2 softplus(0)), so of the two only g's value says anything about that pass
    dead = np.log(2.0) ** 2 + 2 * np.log(2.0)
    assert np.all(pc.case("f")["value64"] == dead) and (pc.case("g")["value64"] != dead).sum() >= 4
    assert 2 * pc.CONFIGS["g"]["channels"] > T


@pytest.mark.parametrize("name", pc.EDGE_NAMES)
def test_edge_seeds_give_the_room_of_the_first_cases(name):
    """The condition under which the generator kept a seed, from the fixture's own arrays: d32 > 0, and the float32 NumPy run of the
    plan (another fp32 summation order, on the CPU) within 2 d32 of ref64 on prior and value."""
    from ipp_rl_amd.planning.mcts_zero.networks import build_plan, run_plan_numpy

    case = pc.case(name)
    assert case["d32_prior"] > 0 and case["d32_value"] > 0 and all(d > 0 for d in case["tap_d32"])
    assert case["seed"] >= case["cfg"]["seed"]
    plan, w = build_plan(case["hp"], case["md"], case["state_dict"], case["cfg"]["side"])
    prior, value = run_plan_numpy(plan, w, case["planes"], case["valid_idx"], dtype=np.float32)
    r_p, r_v = np.abs(prior - case["prior64"]).max() / case["d32_prior"], np.abs(value - case["value64"]).max() / case["d32_value"]
    print(f"{name}: seed {case['seed']}: float32 NumPy plan vs ref64: prior {r_p:.2f} d32, value {r_v:.2f} d32")
    assert r_p <= 2 and r_v <= 2


def test_folding_uses_each_batchnorms_own_eps():
    from ipp_rl_amd.planning.mcts_zero.networks import build_plan

    case = pc.case("c")
    sd = case["state_dict"]
    plan, w = build_plan(case["hp"], case["md"], sd, 9, dtype=np.float64)
    key = "encoder.separable_residual_block_s1"
    off, n = plan.packed[key + ".conv1x3_1:b"]
    s = sd[key + ".bn1.weight"].double() / torch.sqrt(sd[key + ".bn1.running_var"].double() + 1e-3)
    want = (sd[key + ".conv1x3_1.bias"].double() - sd[key + ".bn1.running_mean"].double()) * s + sd[key + ".bn1.bias"].double()
    assert np.abs(w[off:off + n] - want.numpy()).max() < 1e-15
    off, n = plan.packed["encoder.down_sample_block.0.0:b"]
    s = sd["encoder.down_sample_block.0.1.weight"].double() / torch.sqrt(sd["encoder.down_sample_block.0.1.running_var"].double() + 1e-5)
    want = -sd["encoder.down_sample_block.0.1.running_mean"].double() * s + sd["encoder.down_sample_block.0.1.bias"].double()
    assert np.abs(w[off:off + n] - want.numpy()).max() < 1e-15


def test_bf16_rounding_is_nearest_even():
    from ipp_rl_amd.planning.mcts_zero.networks import round_bf16

    x = np.array([1.0, 1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, 1.0 + 2.0 ** -8 + 2.0 ** -20, -0.3, 0.0], dtype=np.float32)
    want = torch.from_numpy(x).to(torch.bfloat16).float().numpy()
    assert np.array_equal(round_bf16(x), want) and round_bf16(x)[1] == 1.0 and round_bf16(x)[2] == np.float32(1.0 + 2.0 ** -6)
    r = np.random.RandomState(0).normal(size=4096).astype(np.float32)
    assert np.array_equal(round_bf16(r), torch.from_numpy(r).to(torch.bfloat16).float().numpy())


def test_bf16_emulation_moves_the_outputs_by_bf16_sized_amounts():
    from ipp_rl_amd.planning.mcts_zero.networks import build_plan, run_plan_numpy

    case = pc.case("b")
    plan, w = build_plan(case["hp"], case["md"], case["state_dict"], 13)
    prior, value = run_plan_numpy(plan, w, case["planes"], case["valid_idx"], round_operands="bf16")
    e = np.abs(value / case["value64"] - 1).max()
    assert 1e-6 < e < 5e-2 and np.abs(prior - case["prior64"]).max() < 5e-2
    with pytest.raises(ValueError):
        run_plan_numpy(plan, w, case["planes"], case["valid_idx"], round_operands="fp8")


def test_value_errors_fire_before_the_device():
    from ipp_rl_amd.feature_planes import PlaneSpec
    from ipp_rl_amd.planning.mcts_zero import DevicePolicyValueNet, PolicyValueNetwork  # noqa: F401  (both exported)
    from ipp_rl_amd.planning.mcts_zero.networks import PV_CONV, build_plan, check_plan

    case = pc.case("b")
    hp, md, sd = case["hp"], case["md"], case["state_dict"]
    with pytest.raises(ValueError, match="mask_policy_head"):
        build_plan(dict(hp, mask_policy_head=False), md, sd, 13)
    with pytest.raises(ValueError, match="mask_policy_head"):
        DevicePolicyValueNet(dict(hp, mask_policy_head=False), md, sd, side=13, device="cuda:0")
    short = {k: v for k, v in sd.items() if not k.startswith("value_head.head")}
    with pytest.raises(ValueError, match="lacks"):
        DevicePolicyValueNet(hp, md, short, side=13, device="cuda:0")
    with pytest.raises(ValueError, match="not square"):
        DevicePolicyValueNet(hp, md, sd, side=(13, 12), device="cuda:0")
    spec = PlaneSpec.from_params(dict(input_history_length=1, use_fov_input=False, use_action_costs_input=True), dict(min_altitude=8.0, max_altitude=14.0))
    assert spec.channels == 6 != hp["input_channels"]
    with pytest.raises(ValueError, match="input_channels"):
        DevicePolicyValueNet(hp, md, sd, side=13, plane_spec=spec, device="cuda:0")
    # the plan conditions ipp_pvnet_create checks, on their host mirror
    plan, w = build_plan(hp, md, sd, 13)
    for field, value, msg in (("kind", 9, "unknown"), ("src", 5, "out of range"), ("hin", 99, "chain"), ("w_off", w.size + 1, "beyond")):
        i = [j for j, op in enumerate(plan.ops) if op["kind"] == PV_CONV][2]
        old = plan.ops[i][field]
        plan.ops[i][field] = value
        with pytest.raises(ValueError, match=msg):
            check_plan(plan, w.size)
        plan.ops[i][field] = old
    check_plan(plan, w.size)


def test_binding_mirrors_the_header():
    import ctypes
    import os
    import re

    from ipp_rl_amd import _ffi
    from ipp_rl_amd.planning.mcts_zero import networks as nw

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    txt = open(os.path.join(root, "include", "ipp_engine.h")).read()
    body = re.search(r"typedef struct ipp_pvnet_op \{(.*?)\} ipp_pvnet_op;", txt, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for typ, names in re.findall(r"(int32_t|int64_t)\s+([a-z_0-9, ]+);", body):
        fields += [(n.strip(), ctypes.c_int32 if typ == "int32_t" else ctypes.c_int64) for n in names.split(",")]
    assert fields == list(nw.IppPvnetOp._fields_) and ctypes.sizeof(nw.IppPvnetOp) == 16 * 4 + 4 * 8
    for macro, val in (("IPP_PV_FP32", nw.PV_FP32), ("IPP_PV_BF16", nw.PV_BF16), ("IPP_PV_OP_CONV", nw.PV_CONV), ("IPP_PV_OP_MIX", nw.PV_MIX),
                       ("IPP_PV_OP_POOL", nw.PV_POOL), ("IPP_PV_OP_VALUE", nw.PV_VALUE), ("IPP_PV_OP_POLICY", nw.PV_POLICY),
                       ("IPP_PV_ACT_RELU", nw.PV_ACT_RELU), ("IPP_PV_ACT_SILU", nw.PV_ACT_SILU)):
        assert int(re.search(rf"#define\s+{macro}\s+(\d+)", txt).group(1)) == val
    plain = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    for name in ("ipp_pvnet_create", "ipp_pvnet_set_weights", "ipp_pvnet_forward", "ipp_pvnet_destroy"):
        m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", plain)
        assert m and len([a for a in m.group(1).split(",") if a.strip()]) == len(_ffi.PROTOTYPES[name][1]), name
    # an invalid plan fails in create, with a message, before any device call
    lib = _ffi.load()
    case = pc.case("b")
    plan, w = nw.build_plan(case["hp"], case["md"], case["state_dict"], 13)
    for field, value, msg in (("kind", 9, b"unknown"), ("dst", 7, b"out of range"), ("win", 99, b"chain"), ("b_off", w.size, b"beyond")):
        ops = [dict(op) for op in plan.ops]
        ops[3][field] = value
        arr = (nw.IppPvnetOp * len(ops))(*[nw.IppPvnetOp(**op) for op in ops])
        net = ctypes.c_void_p()
        assert lib.ipp_pvnet_create(arr, len(ops), w.ctypes.data, w.size, nw.PV_FP32, 4, 0, ctypes.byref(net)) < 0 and not net
        assert msg in lib.ipp_last_error(), (field, lib.ipp_last_error())
