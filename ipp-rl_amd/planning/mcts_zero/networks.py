"""
The policy-value network of the MCTS-zero loop: the trainable module, its inference plan and the device engine that runs the plan.

  PolicyValueNetwork     what planning/mcts_zero/networks/policy_value_networks.py and planning/common/layers.py of the reference
                         compute, restated: same submodule and parameter names (a reference checkpoint loads with strict=True), same
                         forward (x, valid_actions_msk) -> (log_policy, value, reward, decoder).  The training-side object (training.Trainer
                         trains it through forward_logits) and the oracle of the tests; the search's hot path does not use it.
  build_plan             an eval-mode network as a flat list of op records and ONE packed weight blob: every BatchNorm folded into
                         the conv in front of it (running statistics, affine, its own eps), weights the network shares packed once.
                         Dropout, the decoder and the reward output are not planned: predict() discards them
                         (policy_value_network_wrappers.py:217-231).
  run_plan_numpy         the plan interpreted in NumPy: the CPU proof of folding and op order, and with round_operands="bf16" the
                         emulation the bf16 kernels are measured against.
  DevicePolicyValueNet   the plan on the device (csrc/k_pvnet.h through ipp_pvnet_*): `infer` of DeviceMCTS / SelfPlay.

Internal activation layout of the plan is channel-innermost ([n][H][W][C]); the first conv reads the [n][C][N][N] planes of
ipp_feature_planes.  Buffer ids 0..2 are the engine's activation buffers, PV_INPUT the planes; pooled vectors go to slots 0 (policy
trunk) and 1 (value trunk).
"""
import ctypes as C
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Tuple

import numpy as np
import torch
from torch import nn

PV_CONV, PV_MIX, PV_POOL, PV_VALUE, PV_POLICY = 0, 1, 2, 3, 4
PV_ACT_NONE, PV_ACT_RELU, PV_ACT_SILU = 0, 1, 2
PV_INPUT = -1
PV_FP32, PV_BF16 = 0, 1
STRIDE2_BLOCKS = (0, 1, 3, 5)  # Encoder.forward: stride = 2 if i in [0, 1, 3, 5] else 1
SEPARABLE_BN_EPS = 1e-3        # NonBottleneck1d's bn1 / bn2; every other BatchNorm keeps the default 1e-5


# ------------------------------------------------------------------------------------------------------------------ the module
def _conv_then_bn(c_in, c_out, k, **kw):
    return nn.Sequential(nn.Conv2d(c_in, c_out, k, bias=False, **kw), nn.BatchNorm2d(c_out))


class _AvgMaxPool(nn.Module):
    """[n, C, H, W] -> [n, 2C]: the mean over the pixels, then the maximum."""

    def __init__(self):
        super().__init__()
        self.global_avg_pooling = nn.Sequential(nn.AdaptiveAvgPool2d((1, 1)), nn.Flatten())
        self.global_max_pooling = nn.Sequential(nn.AdaptiveMaxPool2d((1, 1)), nn.Flatten())

    def forward(self, x):
        return torch.cat([self.global_avg_pooling(x), self.global_max_pooling(x)], dim=1)


class _Residual(nn.Module):
    """Two 3x3 conv+BN with a biased 1x1 conv on the skip path."""

    def __init__(self, channels, dropout, stride, act):
        super().__init__()
        self.nonlinearity = act
        self.dropout = nn.Dropout2d(dropout)
        self.intermediate_block = nn.Sequential(_conv_then_bn(channels, channels, 3, stride=stride, padding=1), act,
                                                _conv_then_bn(channels, channels, 3, stride=1, padding=1))
        self.conv_identity = nn.Conv2d(channels, channels, 1, stride=stride)

    def forward(self, x):
        y = self.intermediate_block(x)
        if self.dropout.p > 0:
            y = self.dropout(y)
        return self.nonlinearity(y + self.conv_identity(x))


class _SeparableResidual(nn.Module):
    """ERFNet's non-bottleneck-1d block: 3x1, 1x3, BN, 3x1, 1x3, BN around a skip; optionally behind a strided 1x1 conv+BN."""

    def __init__(self, channels, dropout, act, down_sample):
        super().__init__()
        self.down_sample = down_sample
        self.down_sample_layer = nn.Sequential(nn.Conv2d(channels, channels, 1, stride=2, bias=False), nn.BatchNorm2d(channels), act)
        self.conv_identity = nn.Conv2d(channels, channels, 1)
        self.conv3x1_1 = nn.Conv2d(channels, channels, (3, 1), padding=(1, 0))
        self.conv1x3_1 = nn.Conv2d(channels, channels, (1, 3), padding=(0, 1))
        self.conv3x1_2 = nn.Conv2d(channels, channels, (3, 1), padding=(1, 0))
        self.conv1x3_2 = nn.Conv2d(channels, channels, (1, 3), padding=(0, 1))
        self.bn1 = nn.BatchNorm2d(channels, eps=SEPARABLE_BN_EPS)
        self.bn2 = nn.BatchNorm2d(channels, eps=SEPARABLE_BN_EPS)
        self.dropout = nn.Dropout2d(dropout)
        self.nonlinearity = act

    def forward(self, x):
        act = self.nonlinearity
        if self.down_sample:
            x = self.down_sample_layer(x)
        x = self.conv_identity(x)
        y = act(self.bn1(self.conv1x3_1(act(self.conv3x1_1(x)))))
        y = self.bn2(self.conv1x3_2(act(self.conv3x1_2(y))))
        if self.dropout.p > 0:
            y = self.dropout(y)
        return act(y + x)


class _ContextMix(nn.Module):
    """A 3x3 conv whose first G output channels are pooled over the map (after BN and the nonlinearity) and, through a linear
    layer, added to the other channels; then conv+BN and the skip."""

    def __init__(self, channels, act, dropout, pooled_channels, stride=1):
        super().__init__()
        self.stride = stride
        self.nonlinearity = act
        self.num_global_pooling_channels = pooled_channels
        self.conv1 = nn.Conv2d(channels, channels, 3, bias=False, stride=stride, padding=1)
        self.conv_bn_layer_s1 = _conv_then_bn(channels, channels, 3, stride=1, padding=1)
        self.conv_identity = nn.Conv2d(channels, channels, 1, stride=stride)
        self.global_pooling = _AvgMaxPool()
        self.fc_layer = nn.Sequential(nn.Linear(2 * pooled_channels, channels - pooled_channels), act)
        self.bn_layer = nn.BatchNorm2d(pooled_channels)
        self.dropout = nn.Dropout2d(dropout)

    def forward(self, x):
        g = self.num_global_pooling_channels
        skip = self.conv_identity(x) if self.stride > 1 else x
        y = self.conv1(x)
        context = self.fc_layer(self.global_pooling(self.nonlinearity(self.bn_layer(y[:, :g]))))
        y = torch.cat([y[:, :g], y[:, g:] + context[:, :, None, None]], dim=1)
        y = self.conv_bn_layer_s1(y)
        if self.dropout.p > 0:
            y = self.dropout(y)
        return self.nonlinearity(y + skip)


class _Encoder(nn.Module):
    def __init__(self, c_in, channels, act, blocks, dropout, separable, mixing, pooled_channels):
        super().__init__()
        self.num_encoder_res_blocks = blocks
        self.use_separable_conv_layers = separable
        self.use_global_context_mixing = mixing
        self.down_sample_block = nn.Sequential(_conv_then_bn(c_in, channels, 7, stride=2, padding=3), act)
        self.residual_block_s1 = _Residual(channels, dropout, 1, act)
        self.residual_block_s2 = _Residual(channels, dropout, 2, act)
        self.separable_residual_block_s1 = _SeparableResidual(channels, dropout, act, down_sample=False)
        self.separable_residual_block_s2 = _SeparableResidual(channels, dropout, act, down_sample=True)
        self.mix_global_context_s1 = _ContextMix(channels, act, dropout, pooled_channels, stride=1)
        self.mix_global_context_s2 = _ContextMix(channels, act, dropout, pooled_channels, stride=2)

    def block(self, i):
        """The (shared) module that runs as block i, and its attribute name."""
        kind = encoder_block_kind(i, self.use_separable_conv_layers, self.use_global_context_mixing)
        return getattr(self, kind), kind

    def forward(self, x):
        x = self.down_sample_block(x)
        for i in range(self.num_encoder_res_blocks):
            x = self.block(i)[0](x)
        return x


def encoder_block_kind(i: int, separable: bool, mixing: bool) -> str:
    s = 2 if i in STRIDE2_BLOCKS else 1
    if mixing and i > 0 and i % 3 == 0:
        return f"mix_global_context_s{s}"
    return f"separable_residual_block_s{s}" if separable else f"residual_block_s{s}"


class _Decoder(nn.Module):
    def __init__(self, channels, act, dropout):
        super().__init__()
        up = lambda a, b: nn.Sequential(nn.ConvTranspose2d(a, b, 2, stride=2), nn.BatchNorm2d(b), act, nn.Dropout2d(dropout))  # noqa: E731
        self.conv_transpose1 = up(channels, channels // 2)
        self.conv_transpose2 = up(channels // 4, channels // 8)
        self.decoder = nn.Sequential(self.conv_transpose1, _conv_then_bn(channels // 2, channels // 4, 3, stride=1, padding=1), act,
                                     nn.Dropout2d(dropout), self.conv_transpose2, _conv_then_bn(channels // 8, 1, 3, stride=1, padding=1))

    def forward(self, x):
        return self.decoder(x)[:, 0]


class _HeadTrunk(nn.Module):
    """What both heads share: `blocks` rounds of ONE conv+BN block (the first round a context mix instead, when mixing), then
    the average / maximum pool."""

    def __init__(self, channels, blocks, act, dropout, mixing, pooled_channels):
        super().__init__()
        self.num_conv_bn_blocks = blocks
        self.use_global_context_mixing = mixing
        self.dropout = nn.Dropout2d(dropout)
        self.global_pooling_layer = _AvgMaxPool()
        self.conv_bn_block = nn.Sequential(_conv_then_bn(channels, channels, 3, stride=1, padding=1), act)
        self.mix_global_context = _ContextMix(channels, act, dropout, pooled_channels)

    def trunk(self, x):
        for i in range(self.num_conv_bn_blocks):
            if i == 0 and self.use_global_context_mixing:
                x = self.mix_global_context(x)
                continue
            x = self.conv_bn_block(x)
            if self.dropout.p > 0:
                x = self.dropout(x)
        return self.global_pooling_layer(x)


class _ValueHead(_HeadTrunk):
    def __init__(self, channels, blocks, act, dropout, reward, mixing, pooled_channels):
        super().__init__(channels, blocks, act, dropout, mixing, pooled_channels)
        self.use_reward_target = reward
        self.head = nn.Sequential(nn.Linear(2 * channels, 1), act, nn.Softplus())

    def forward(self, x):
        pooled = self.trunk(x)
        return self.head(pooled), (self.head(pooled) if self.use_reward_target else None)


class _PolicyHead(_HeadTrunk):
    def __init__(self, channels, blocks, act, actions, dropout, masked, mixing, pooled_channels):
        super().__init__(channels, blocks, act, dropout, mixing, pooled_channels)
        self.mask_policy_head = masked
        self.head = nn.Sequential(nn.Linear(2 * channels, actions))
        self.output_fn = nn.LogSoftmax(dim=1)

    def logits(self, x):
        return self.head(self.trunk(x))

    def forward(self, x, valid_actions_msk):
        logits = self.logits(x)
        if self.mask_policy_head:
            logits = logits - (1 - valid_actions_msk) * 1000
        return self.output_fn(logits)


def num_actions_of(meta_data: Dict) -> int:
    levels = int((meta_data["max_altitude"] - meta_data["min_altitude"]) / meta_data["altitude_spacing"]) + 1
    return int(meta_data["num_grid_cells"]) * levels


class PolicyValueNetwork(nn.Module):
    def __init__(self, hyper_params: Dict, meta_data: Dict):
        super().__init__()
        hp = self.hyper_params = hyper_params
        self.num_actions = num_actions_of(meta_data)
        self.device = torch.device("cuda" if torch.cuda.is_available() else "cpu")
        act = nn.SiLU() if hp["use_silu"] else nn.ReLU()
        c, drop, mixing, g = hp["num_channels"], hp["dropout"], hp["use_global_context_mixing"], hp["num_global_pooling_channels"]
        self.encoder = _Encoder(hp["input_channels"], c, act, hp["num_encoder_res_blocks"], drop, hp["use_separable_conv_layers"], mixing, g)
        self.policy_head = _PolicyHead(c, hp["num_policy_head_conv_bn_blocks"], act, self.num_actions, drop, hp["mask_policy_head"], mixing, g)
        self.value_head = _ValueHead(c, hp["num_value_head_conv_bn_blocks"], act, drop, hp["use_reward_target"], mixing, g)
        self.decoder = _Decoder(c, act, drop)

    def forward(self, x, valid_actions_msk):
        x = self.encoder(x)
        log_policy = self.policy_head(x, valid_actions_msk)
        value, reward = self.value_head(x)
        return log_policy, value, reward, (self.decoder(x) if self.hyper_params["use_autoencoder"] else None)

    def forward_logits(self, x):
        """(logits, value, reward, decoder): forward without the mask and the LogSoftmax, what ipp_pvnet_loss takes (training.Trainer)."""
        x = self.encoder(x)
        logits = self.policy_head.logits(x)
        value, reward = self.value_head(x)
        return logits, value, reward, (self.decoder(x) if self.hyper_params["use_autoencoder"] else None)


# ------------------------------------------------------------------------------------------------------------------ the plan
@dataclass
class Plan:
    ops: List[Dict] = field(default_factory=list)
    blocks: List[Tuple[str, int]] = field(default_factory=list)  # top-level block -> index of the op that writes its output
    packed: Dict[str, Tuple[int, int]] = field(default_factory=dict)  # packed tensor -> (offset, floats) in the blob
    side: int = 0
    input_channels: int = 0
    num_channels: int = 0
    num_actions: int = 0
    n_floats: int = 0

    def tap(self, name: str) -> int:
        return dict(self.blocks)[name]


OP_FIELDS = ("kind", "kh", "kw", "stride", "pad_h", "pad_w", "cin", "cout", "hin", "win", "hout", "wout", "src", "dst", "res", "act")
OP_OFFSETS = ("w_off", "b_off", "w2_off", "b2_off")


class IppPvnetOp(C.Structure):
    """ipp_pvnet_op (include/ipp_engine.h)."""
    _fields_ = [(f, C.c_int32) for f in OP_FIELDS] + [(f, C.c_int64) for f in OP_OFFSETS]


def required_keys(hyper_params: Dict, meta_data: Dict) -> List[str]:
    with torch.device("meta"):
        return list(PolicyValueNetwork(hyper_params, meta_data).state_dict().keys())


class _Builder:
    def __init__(self, sd, act, side, dtype):
        self.sd, self.act, self.dtype = sd, act, dtype
        self.plan = Plan(side=side)
        self.chunks, self.n = [], 0

    def t(self, key):
        v = self.sd[key]
        return (v.detach().cpu().double().numpy() if torch.is_tensor(v) else np.asarray(v, dtype=np.float64))

    def put(self, key, make):
        """Offset of the packed tensor `key`; packed by make() the first time it is asked for."""
        if key not in self.plan.packed:
            a = np.ascontiguousarray(make(), dtype=np.float64).reshape(-1)
            self.plan.packed[key] = (self.n, a.size)
            self.chunks.append(a)
            self.n += a.size
        return self.plan.packed[key][0]

    def bn(self, key, eps):
        """Eval-mode BatchNorm as (scale, shift)."""
        s = self.t(key + ".weight") / np.sqrt(self.t(key + ".running_var") + eps)
        return s, self.t(key + ".bias") - self.t(key + ".running_mean") * s

    def conv(self, key, src, dst, hw, stride=1, act=PV_ACT_NONE, res=-1, bn=None, eps=1e-5):
        w = self.t(key + ".weight")  # [co, ci, kh, kw]
        co, ci, kh, kw = w.shape
        ph, pw = kh // 2, kw // 2

        def folded():
            b = self.t(key + ".bias") if (key + ".bias") in self.sd else np.zeros(co)
            if bn is None:
                return w, b
            s, sh = self.bn(bn, eps)
            return w * s[:, None, None, None], b * s + sh

        h, wd = hw
        ho, wo = (h + 2 * ph - kh) // stride + 1, (wd + 2 * pw - kw) // stride + 1
        self.plan.ops.append(dict(kind=PV_CONV, kh=kh, kw=kw, stride=stride, pad_h=ph, pad_w=pw, cin=ci, cout=co, hin=h, win=wd, hout=ho,
                                  wout=wo, src=src, dst=dst, res=res, act=act,
                                  w_off=self.put(key + ":w", lambda: folded()[0].transpose(0, 2, 3, 1)),  # [co][kh][kw][ci]
                                  b_off=self.put(key + ":b", lambda: folded()[1]), w2_off=0, b2_off=0))
        return ho, wo

    def mix_op(self, key, buf, hw, channels, g):
        self.plan.ops.append(dict(kind=PV_MIX, kh=0, kw=0, stride=0, pad_h=0, pad_w=0, cin=g, cout=channels, hin=hw[0], win=hw[1], hout=hw[0],
                                  wout=hw[1], src=buf, dst=buf, res=-1, act=self.act,
                                  w_off=self.put(key + ".bn_layer:scale", lambda: self.bn(key + ".bn_layer", 1e-5)[0]),
                                  b_off=self.put(key + ".bn_layer:shift", lambda: self.bn(key + ".bn_layer", 1e-5)[1]),
                                  w2_off=self.put(key + ".fc_layer.0:w", lambda: self.t(key + ".fc_layer.0.weight")),  # [C - G][2G]
                                  b2_off=self.put(key + ".fc_layer.0:b", lambda: self.t(key + ".fc_layer.0.bias"))))

    def head_op(self, kind, key, slot, channels, cout, hw=(1, 1), src=None):
        self.plan.ops.append(dict(kind=kind, kh=0, kw=0, stride=0, pad_h=0, pad_w=0, cin=channels, cout=cout, hin=hw[0], win=hw[1], hout=1, wout=1,
                                  src=slot if src is None else src, dst=slot, res=-1, act=self.act if kind == PV_VALUE else PV_ACT_NONE,
                                  w_off=self.put(key + ":w", lambda: self.t(key + ".weight")) if key else 0,
                                  b_off=self.put(key + ":b", lambda: self.t(key + ".bias")) if key else 0, w2_off=0, b2_off=0))

    # blocks: each returns (buffer that holds the result, its extent); `cur` is read, every buffer but `keep` may be written
    def residual(self, key, cur, hw, stride):
        a, b = [i for i in range(3) if i != cur]
        self.conv(key + ".conv_identity", cur, a, hw, stride)
        o = self.conv(key + ".intermediate_block.0.0", cur, b, hw, stride, self.act, bn=key + ".intermediate_block.0.1")
        self.conv(key + ".intermediate_block.2.0", b, cur, o, 1, self.act, res=a, bn=key + ".intermediate_block.2.1")
        return cur, o

    def separable(self, key, cur, hw, down):
        a, b = [i for i in range(3) if i != cur]
        if down:
            hw = self.conv(key + ".down_sample_layer.0", cur, a, hw, 2, self.act, bn=key + ".down_sample_layer.1")
            self.conv(key + ".conv_identity", a, b, hw)
        else:
            self.conv(key + ".conv_identity", cur, b, hw)
        self.conv(key + ".conv3x1_1", b, cur, hw, act=self.act)
        self.conv(key + ".conv1x3_1", cur, a, hw, act=self.act, bn=key + ".bn1", eps=SEPARABLE_BN_EPS)
        self.conv(key + ".conv3x1_2", a, cur, hw, act=self.act)
        self.conv(key + ".conv1x3_2", cur, a, hw, act=self.act, res=b, bn=key + ".bn2", eps=SEPARABLE_BN_EPS)
        return a, hw

    def mix(self, key, cur, hw, stride, channels, g):
        a, b = [i for i in range(3) if i != cur]
        if stride > 1:
            self.conv(key + ".conv_identity", cur, a, hw, stride)
            o = self.conv(key + ".conv1", cur, b, hw, stride)
            self.mix_op(key, b, o, channels, g)
            self.conv(key + ".conv_bn_layer_s1.0", b, cur, o, act=self.act, res=a, bn=key + ".conv_bn_layer_s1.1")
            return cur, o
        self.conv(key + ".conv1", cur, a, hw)
        self.mix_op(key, a, hw, channels, g)
        self.conv(key + ".conv_bn_layer_s1.0", a, b, hw, act=self.act, res=cur, bn=key + ".conv_bn_layer_s1.1")
        return b, hw


def build_plan(hyper_params: Dict, meta_data: Dict, state_dict: Dict, side: int, dtype=np.float32):
    """(plan, weights): the op records of the eval-mode network on side x side planes and the packed blob (`dtype`: float32 for the
    device, float64 for exact checks of the folding)."""
    hp = hyper_params
    if not hp["mask_policy_head"]:
        raise ValueError("mask_policy_head=False needs the softmax normaliser over all actions: not built (the search reads the policy on "
                         "the valid set only)")
    missing = [k for k in required_keys(hp, meta_data) if k not in state_dict]
    if missing:
        raise ValueError(f"state_dict lacks {len(missing)} keys of the network, e.g. {missing[:3]}")
    c, g, mixing = int(hp["num_channels"]), int(hp["num_global_pooling_channels"]), bool(hp["use_global_context_mixing"])
    act = PV_ACT_SILU if hp["use_silu"] else PV_ACT_RELU
    bld = _Builder(state_dict, act, int(side), dtype)
    plan = bld.plan
    plan.input_channels, plan.num_channels, plan.num_actions = int(hp["input_channels"]), c, num_actions_of(meta_data)
    if tuple(state_dict["encoder.down_sample_block.0.0.weight"].shape[:2]) != (c, plan.input_channels):
        raise ValueError("state_dict does not belong to a network of these hyper_params (stem shape)")
    if tuple(state_dict["policy_head.head.0.weight"].shape) != (plan.num_actions, 2 * c):
        raise ValueError("state_dict does not belong to a network of this meta_data (policy head shape)")

    cur = 0
    hw = bld.conv("encoder.down_sample_block.0.0", PV_INPUT, cur, (side, side), 2, act, bn="encoder.down_sample_block.0.1")
    plan.blocks.append(("encoder.down_sample_block", len(plan.ops) - 1))
    for i in range(int(hp["num_encoder_res_blocks"])):
        kind = encoder_block_kind(i, bool(hp["use_separable_conv_layers"]), mixing)
        key, stride = "encoder." + kind, int(kind[-1])
        if kind.startswith("mix"):
            cur, hw = bld.mix(key, cur, hw, stride, c, g)
        elif kind.startswith("separable"):
            cur, hw = bld.separable(key, cur, hw, stride == 2)
        else:
            cur, hw = bld.residual(key, cur, hw, stride)
        plan.blocks.append((f"encoder.block{i}", len(plan.ops) - 1))
    enc = cur
    for slot, head, n_blocks in ((0, "policy_head", int(hp["num_policy_head_conv_bn_blocks"])), (1, "value_head", int(hp["num_value_head_conv_bn_blocks"]))):
        t = enc
        for i in range(n_blocks):
            if i == 0 and mixing:
                t, _ = bld.mix(head + ".mix_global_context", enc, hw, 1, c, g)  # (stride 1: reads enc, writes the two others)
            else:
                dst = [b for b in range(3) if b != enc and b != t][0]
                bld.conv(head + ".conv_bn_block.0.0", t, dst, hw, act=act, bn=head + ".conv_bn_block.0.1")
                t = dst
            plan.blocks.append((f"{head}.block{i}", len(plan.ops) - 1))
        bld.head_op(PV_POOL, None, slot, c, 2 * c, hw, src=t)
    bld.head_op(PV_VALUE, "value_head.head.0", 1, c, 1)
    bld.head_op(PV_POLICY, "policy_head.head.0", 0, c, plan.num_actions)
    plan.n_floats = bld.n
    return plan, np.concatenate(bld.chunks).astype(dtype)


def check_plan(plan: Plan, n_floats: int) -> None:
    """A SUBSET of what ipp_pvnet_create checks (csrc/ipp_pvnet.hip validate(), the authority: it also checks residual shapes, pooled
    slots, kernel extents and every tensor's extent, before any device call), so that a plan edited by hand fails in Python with a
    ValueError: op kinds, buffer ids, the chain of input shapes and the weight offsets."""
    shape = {}
    for i, op in enumerate(plan.ops):
        if op["kind"] not in (PV_CONV, PV_MIX, PV_POOL, PV_VALUE, PV_POLICY):
            raise ValueError(f"op {i}: unknown kind {op['kind']}")
        if op["kind"] in (PV_CONV, PV_MIX, PV_POOL):
            if not (op["src"] == PV_INPUT and i == 0) and not 0 <= op["src"] < 3:
                raise ValueError(f"op {i}: buffer id {op['src']} out of range")
            if op["src"] != PV_INPUT and shape.get(op["src"]) != (op["hin"], op["win"], op["cin"] if op["kind"] != PV_MIX else op["cout"]):
                raise ValueError(f"op {i}: input shape does not chain")
        if op["kind"] == PV_CONV:
            if not 0 <= op["dst"] < 3 or op["dst"] == op["src"] or op["res"] == op["dst"]:
                raise ValueError(f"op {i}: bad output buffer")
            shape[op["dst"]] = (op["hout"], op["wout"], op["cout"])
        for f in OP_OFFSETS:
            if not 0 <= op[f] <= n_floats:
                raise ValueError(f"op {i}: weight offset beyond the blob")


def round_bf16(x: np.ndarray) -> np.ndarray:
    """float32 values rounded to the nearest bfloat16, ties to even (as float32)."""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    u = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16) << 16
    return u.astype(np.uint32).view(np.float32).reshape(np.shape(x))


def _act(x, kind):
    if kind == PV_ACT_RELU:
        return np.maximum(x, 0)
    if kind == PV_ACT_SILU:
        return x / (1 + np.exp(-x))
    return x


def run_plan_numpy(plan: Plan, weights: np.ndarray, planes: np.ndarray, valid_idx: np.ndarray, dtype=np.float64, round_operands: Optional[str] = None,
                   tap_op: int = -1):
    """(prior [n, kmax], value [n]) of the plan in `dtype`; with tap_op the [n, C', H', W'] output of that op as a third item.
    round_operands="bf16": every conv / linear operand (activations and weights) is rounded to bfloat16 first; sums stay in `dtype`."""
    if round_operands not in (None, "bf16"):
        raise ValueError("round_operands: None or 'bf16'")
    rd = (lambda a: round_bf16(a).astype(dtype)) if round_operands else (lambda a: a)
    wts = np.asarray(weights)
    W = lambda off, n: wts[off:off + n].astype(dtype)  # noqa: E731
    n = planes.shape[0]
    bufs, pooled, tap = {PV_INPUT: np.transpose(planes, (0, 2, 3, 1)).astype(dtype)}, {}, None
    prior = value = None
    for i, op in enumerate(plan.ops):
        k = op["kind"]
        if k == PV_CONV:
            x = rd(bufs[op["src"]])
            kh, kw, s, ci, co = op["kh"], op["kw"], op["stride"], op["cin"], op["cout"]
            xp = np.pad(x, ((0, 0), (op["pad_h"],) * 2, (op["pad_w"],) * 2, (0, 0)))
            ho, wo = op["hout"], op["wout"]
            wk = rd(W(op["w_off"], co * kh * kw * ci)).reshape(co, kh * kw, ci)
            y = np.zeros((n * ho * wo, co), dtype=dtype) + W(op["b_off"], co)
            for tp in range(kh * kw):  # one [pixels, ci] x [ci, co] product per tap: no im2col copy of a large plane
                ky, kx = divmod(tp, kw)
                y += xp[:, ky:ky + s * (ho - 1) + 1:s, kx:kx + s * (wo - 1) + 1:s, :].reshape(-1, ci) @ wk[:, tp, :].T
            y = y.reshape(n, ho, wo, co)
            if op["res"] >= 0:
                y = y + bufs[op["res"]]
            bufs[op["dst"]] = _act(y, op["act"])
        elif k == PV_MIX:
            g, c = op["cin"], op["cout"]
            x = bufs[op["src"]]
            p = _act(x[..., :g] * W(op["w_off"], g) + W(op["b_off"], g), op["act"]).reshape(n, -1, g)
            pv = np.concatenate([p.mean(axis=1), p.max(axis=1)], axis=1)
            ctx = _act(rd(pv) @ rd(W(op["w2_off"], (c - g) * 2 * g)).reshape(c - g, 2 * g).T + W(op["b2_off"], c - g), op["act"])
            bufs[op["dst"]] = np.concatenate([x[..., :g], x[..., g:] + ctx[:, None, None, :]], axis=3)
        elif k == PV_POOL:
            x = bufs[op["src"]].reshape(n, -1, op["cin"])
            pooled[op["dst"]] = np.concatenate([x.mean(axis=1), x.max(axis=1)], axis=1)
        elif k == PV_VALUE:
            z = _act(rd(pooled[op["src"]]) @ rd(W(op["w_off"], 2 * op["cin"])) + W(op["b_off"], 1)[0], op["act"])
            v = np.where(z > 20, z, np.log1p(np.exp(np.minimum(z, 20))))  # nn.Softplus
            value = v * v + 2 * v
        elif k == PV_POLICY:
            c2, kmax = 2 * op["cin"], valid_idx.shape[1]
            wp, bp, pv = W(op["w_off"], op["cout"] * c2).reshape(op["cout"], c2), W(op["b_off"], op["cout"]), rd(pooled[op["src"]])
            prior = np.zeros((n, kmax), dtype=np.float64)
            for r in range(n):
                ids = valid_idx[r][valid_idx[r] >= 0]
                if len(ids):
                    lg = (rd(wp[ids]) @ pv[r] + bp[ids]).astype(np.float64)
                    e = np.exp(lg - lg.max())
                    prior[r, :len(ids)] = e / e.sum()
        if i == tap_op:
            tap = np.transpose(bufs[op["dst"]], (0, 3, 1, 2)).copy()
    out = (prior, np.asarray(value, dtype=np.float64))
    return out + (tap,) if tap_op >= 0 else out


# ------------------------------------------------------------------------------------------------------------------ the device engine
class DevicePolicyValueNet:
    """The network on the device: predict(planes, valid_idx) -> (prior [n, kmax] f64, value [n] f64), both device tensors, on the
    current stream; `infer` is the callback of DeviceMCTS(feature_planes=True) / SelfPlay."""

    def __init__(self, hyper_params: Dict, meta_data: Dict, state_dict: Dict, side: int, precision: str = "fp32", max_batch: int = 4096,
                 device="cuda:0", plane_spec=None):
        # ipp_feature_planes' planes are [n, C, N, N] with N = the number of grid cells (the covariance as an image), whatever the grid's
        # own shape: for an engine's planes side = cfg.n_cells.  A pair (height, width) is taken so that a mismatch is named, not guessed.
        if isinstance(side, (tuple, list)):
            if len(side) != 2 or int(side[0]) != int(side[1]):
                raise ValueError(f"the network's planes are square: the grid of planes is not square: {tuple(side)}")
            side = side[0]
        if int(side) < 1:
            raise ValueError("side < 1")
        if plane_spec is not None and int(plane_spec.channels) != int(hyper_params["input_channels"]):
            raise ValueError(f"input_channels = {hyper_params['input_channels']}, the feature planes have {plane_spec.channels} channels")
        if precision not in ("fp32", "bf16"):
            raise ValueError("precision: 'fp32' or 'bf16'")
        if max_batch < 1:
            raise ValueError("max_batch < 1")
        self.hyper_params, self.meta_data, self.side, self.precision, self.max_batch = hyper_params, meta_data, int(side), precision, int(max_batch)
        self.plan, weights = build_plan(hyper_params, meta_data, state_dict, side)  # ValueError: missing keys, dense policy head
        check_plan(self.plan, weights.size)
        from ... import _ffi

        self._ffi, self._lib = _ffi, _ffi.load()
        self.device = torch.device(device)
        ops = (IppPvnetOp * len(self.plan.ops))(*[IppPvnetOp(**op) for op in self.plan.ops])
        self._net = C.c_void_p()
        self._busy = None  # event after the last forward: the handle's activation buffers serve one forward at a time
        _ffi.check(self._lib.ipp_pvnet_create(ops, len(self.plan.ops), weights.ctypes.data, weights.size, PV_BF16 if precision == "bf16" else PV_FP32,
                                              self.max_batch, self.device.index or 0, C.byref(self._net)))

    def _stream(self):
        return torch.cuda.current_stream(self.device).cuda_stream

    def load_state_dict(self, state_dict: Dict) -> None:
        """Re-fold and upload (the trainer's hand-over); the architecture stays."""
        plan, weights = build_plan(self.hyper_params, self.meta_data, state_dict, self.side)
        if plan.ops != self.plan.ops:
            raise ValueError("state_dict of another architecture")
        if self._busy is not None:
            torch.cuda.current_stream(self.device).wait_event(self._busy)
        self._ffi.check(self._lib.ipp_pvnet_set_weights(self._net, weights.ctypes.data, weights.size, self._stream()))

    def predict(self, planes, valid_idx, tap_op: int = -1):
        p = self.plan
        if planes.dim() != 4 or tuple(planes.shape[1:]) != (p.input_channels, p.side, p.side) or planes.dtype != torch.float32:
            raise ValueError(f"planes: float32 [n, {p.input_channels}, {p.side}, {p.side}], got {planes.dtype} {tuple(planes.shape)}")
        n = planes.shape[0]
        if valid_idx.dim() != 2 or valid_idx.shape[0] != n:
            raise ValueError("valid_idx: [n, kmax]")
        planes = planes.to(self.device).contiguous()
        idx = valid_idx.to(device=self.device, dtype=torch.int32).contiguous()
        kmax = idx.shape[1]
        prior = torch.empty((n, kmax), dtype=torch.float64, device=self.device)
        value = torch.empty((n,), dtype=torch.float64, device=self.device)
        tap = None
        if tap_op >= 0:
            op = p.ops[tap_op]
            if op["kind"] != PV_CONV:
                raise ValueError("tap_op: a conv op")
            tap = torch.empty((n, op["cout"], op["hout"], op["wout"]), dtype=torch.float32, device=self.device)
        if n:
            # DeviceMCTS(groups=2) calls from two streams whose waves overlap: a forward waits for the one before it
            cur = torch.cuda.current_stream(self.device)
            if self._busy is not None:
                cur.wait_event(self._busy)
            self._ffi.check(self._lib.ipp_pvnet_forward(self._net, planes.data_ptr(), n, idx.data_ptr(), kmax, prior.data_ptr(), value.data_ptr(),
                                                        int(tap_op), tap.data_ptr() if tap is not None else None, self._stream()))
            self._busy = torch.cuda.Event()
            self._busy.record(cur)
        return (prior, value, tap) if tap_op >= 0 else (prior, value)

    def infer(self, batch):
        return self.predict(batch["planes"], batch["valid_idx"])

    def close(self):
        if getattr(self, "_net", None) is not None and self._net:
            self._lib.ipp_pvnet_destroy(self._net)
            self._net = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
