"""Shared by the CPU and GPU DeepSeek-V3 block tests: a randomly initialised tiny DeepSeek-V3 (transformers 5 layout: one dense layer, then one MoE layer
with 3-D expert parameters, a sigmoid / group-limited ``DeepseekV3TopkRouter`` with its ``e_score_correction_bias`` and an always-on ``shared_experts``
SwiGLU MLP), its routed experts and shared experts quantised with the oracle's min/max quantizer, packed (pack_model + pack_moe_experts), saved under the
names transformers gives (``mlp.experts.{e}.gate_proj / up_proj / down_proj``, ``mlp.shared_experts.*``; the router ``mlp.gate``, the attention and the dense
layer stay dense), and its dequantised fp16 twin.  Modelled on _tiny_qwen2_moe.py."""
import torch

from oracle import gptq_oracle as O

from _tiny_mixtral import _quant
from _tiny_qwen2_moe import save_checkpoint  # noqa: F401  (the same checkpoint layout)

BITS, GROUP = 4, 64
H, I, N_SHARED, E, TOPK, N_GROUP, TOPK_GROUP, SCALE = 256, 128, 2, 16, 4, 4, 2, 2.5
I_S = I * N_SHARED
NAMES = ("gate_proj", "up_proj", "down_proj")


def tiny_config():
    from transformers import DeepseekV3Config
    return DeepseekV3Config(hidden_size=H, intermediate_size=512, moe_intermediate_size=I, num_hidden_layers=2, num_attention_heads=4,
                            num_key_value_heads=4, n_shared_experts=N_SHARED, n_routed_experts=E, routed_scaling_factor=SCALE, kv_lora_rank=64,
                            q_lora_rank=128, qk_rope_head_dim=64, v_head_dim=64, qk_nope_head_dim=64, n_group=N_GROUP, topk_group=TOPK_GROUP,
                            num_experts_per_tok=TOPK, first_k_dense_replace=1, norm_topk_prob=True, vocab_size=512, max_position_embeddings=128,
                            attn_implementation="sdpa", tie_word_embeddings=False)


def moe_blocks(model):
    return [layer.mlp for layer in model.model.layers if type(layer.mlp).__name__ == "DeepseekV3MoE"]


def fresh_model(seed):
    from transformers import DeepseekV3ForCausalLM
    torch.manual_seed(seed)
    m = DeepseekV3ForCausalLM(tiny_config())
    m.lm_head.weight.data.normal_(0, 0.3)
    for mod in m.modules():                        # transformers leaves the 3-D expert parameters uninitialised: give them a scale like the linears'
        if hasattr(mod, "gate_up_proj") and torch.is_tensor(mod.gate_up_proj):
            mod.gate_up_proj.data.normal_(0, 0.05)
            mod.down_proj.data.normal_(0, 0.05)
        if type(mod).__name__ == "DeepseekV3TopkRouter":
            mod.weight.data.normal_(0, 0.05)
            mod.e_score_correction_bias.data.normal_(0, 0.05)      # zeros by default: the bias path would go untested
    return m.half().eval()


def quantize_and_pack(model, desc_act=False, seed=0):
    """Shared-expert linears through pack_model, routed experts through pack_moe_experts.  Returns the twin's weights {state-dict key: dequantised tensor}
    computed by the ORACLE from the packed tensors (linears: [N, K]; experts: the 3-D gate_up_proj / down_proj)."""
    from autogptq_amd.model_utils import find_layers, pack_model
    from autogptq_amd.moe import dense_expert_modules, pack_moe_experts

    gen = torch.Generator().manual_seed(seed)
    lin = {n: l for n, l in find_layers(model).items() if n.startswith("model.layers.") and ".shared_experts." in n}
    quantizers = {n: _quant(l.weight.data, desc_act, gen) for n, l in lin.items()}
    ex_q = {}
    dense = dense_expert_modules(model)
    for path, m in dense.items():
        for e in range(m.num_experts):
            gu, dn = m.gate_up_proj.data[e], m.down_proj.data[e]
            for nm, W in zip(NAMES, (gu[:I], gu[I:], dn)):
                ex_q[f"{path}.{e}.{nm}"] = _quant(W, desc_act, gen)
    pack_model(model, quantizers, BITS, GROUP, desc_act=desc_act)
    pack_moe_experts(model, ex_q, BITS, GROUP, desc_act=desc_act, names=NAMES)
    mode = O.reference_zero_mode(desc_act, BITS)

    def dq(q):
        return O.dequantize(q.qweight.cpu(), q.qzeros.cpu(), q.scales.cpu(), q.g_idx.cpu(), BITS, mode)      # [K, N]

    twin_w = {n + ".weight": dq(model.get_submodule(n)).t().contiguous() for n in quantizers}
    for path in dense:
        q = model.get_submodule(path)
        twin_w[path + ".gate_up_proj"] = torch.stack([torch.cat([dq(q[e].gate_proj).t(), dq(q[e].up_proj).t()], 0) for e in range(E)]).contiguous()
        twin_w[path + ".down_proj"] = torch.stack([dq(q[e].down_proj).t() for e in range(E)]).contiguous()
    return twin_w


def load_checkpoint(path, seed=99):
    import json
    import os
    from safetensors.torch import load_file
    from autogptq_amd.model_utils import load_packed_layers

    with open(os.path.join(path, "quantize_config.json")) as f:
        qc = json.load(f)
    sd = load_file(os.path.join(path, "model.safetensors"))
    model = fresh_model(seed)
    return load_packed_layers(model, sd, qc["bits"], qc["group_size"], desc_act=qc["desc_act"], quant_method=qc["quant_method"],
                              checkpoint_format=qc["checkpoint_format"]), sd, qc


def make_twin(src_state, twin_w, seed=7):
    """fp16 DeepSeek-V3 whose quantised weights are the dequantised ones and whose other tensors (the router's correction bias included) equal the
    quantised model's."""
    twin = fresh_model(seed)
    sd = twin.state_dict()
    for k in sd:
        if k in src_state and src_state[k].shape == sd[k].shape and src_state[k].dtype == sd[k].dtype:
            sd[k] = src_state[k].clone()
    for k, W in twin_w.items():
        sd[k] = W.to(sd[k].dtype).clone()
    twin.load_state_dict(sd)
    return twin


def build(tmp_path, desc_act=False):
    """(quantised model reloaded through load_packed_layers, fp16 twin), both on the CPU."""
    src = fresh_model(0)
    twin_w = quantize_and_pack(src, desc_act)
    save_checkpoint(src, str(tmp_path), desc_act)
    model, _, _ = load_checkpoint(str(tmp_path))
    twin = make_twin(model.state_dict(), twin_w)
    return model, twin
