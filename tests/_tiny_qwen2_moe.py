"""Shared by the CPU and GPU shared-expert tests: a randomly initialised tiny Qwen2-MoE (transformers 5 layout: 3-D expert parameters, a SwiGLU
``shared_expert`` and a dense ``shared_expert_gate`` in every block), its attention linears, routed experts and shared experts quantised with the oracle's
min/max quantizer, packed (pack_model + pack_moe_experts), saved under the names transformers gives (``mlp.experts.{e}.gate_proj / up_proj / down_proj``,
``mlp.shared_expert.*``; ``mlp.shared_expert_gate`` and the router ``mlp.gate`` stay dense), and its dequantised fp16 twin.  Modelled on _tiny_mixtral.py."""
import json
import os

import torch

from oracle import gptq_oracle as O

from _tiny_mixtral import _quant

BITS, GROUP = 4, 64
H, I, I_S, E, TOPK = 256, 128, 320, 8, 2
NAMES = ("gate_proj", "up_proj", "down_proj")


def tiny_config():
    from transformers import Qwen2MoeConfig
    return Qwen2MoeConfig(hidden_size=H, intermediate_size=512, moe_intermediate_size=I, shared_expert_intermediate_size=I_S, num_hidden_layers=2,
                          num_attention_heads=4, num_key_value_heads=4, num_experts=E, num_experts_per_tok=TOPK, decoder_sparse_step=1, mlp_only_layers=[],
                          norm_topk_prob=True, vocab_size=512, max_position_embeddings=128, attn_implementation="sdpa", tie_word_embeddings=False)


def fresh_model(seed):
    from transformers import Qwen2MoeForCausalLM
    torch.manual_seed(seed)
    m = Qwen2MoeForCausalLM(tiny_config())
    m.lm_head.weight.data.normal_(0, 0.3)
    for mod in m.modules():                        # transformers leaves the 3-D expert parameters uninitialised: give them a scale like the linears'
        if hasattr(mod, "gate_up_proj") and torch.is_tensor(mod.gate_up_proj):
            mod.gate_up_proj.data.normal_(0, 0.05)
            mod.down_proj.data.normal_(0, 0.05)
        if type(mod).__name__ == "Qwen2MoeSparseMoeBlock":
            mod.shared_expert_gate.weight.data.normal_(0, 0.05)
            mod.gate.weight.data.normal_(0, 0.05)
    return m.half().eval()


def quantize_and_pack(model, desc_act=False, seed=0):
    """Attention and shared-expert linears through pack_model, routed experts through pack_moe_experts.  Returns the twin's weights {state-dict key:
    dequantised tensor} computed by the ORACLE from the packed tensors (linears: [N, K]; experts: the 3-D gate_up_proj / down_proj)."""
    from autogptq_amd.model_utils import find_layers, pack_model
    from autogptq_amd.moe import dense_expert_modules, pack_moe_experts

    gen = torch.Generator().manual_seed(seed)
    lin = {n: l for n, l in find_layers(model).items() if n.startswith("model.layers.") and (".self_attn." in n or ".shared_expert." in n)}
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


def save_checkpoint(model, path, desc_act=False):
    from safetensors.torch import save_file
    os.makedirs(path, exist_ok=True)
    sd = {k: v.detach().cpu().contiguous() for k, v in model.state_dict().items()}
    save_file(sd, os.path.join(path, "model.safetensors"), metadata={"format": "pt"})
    with open(os.path.join(path, "quantize_config.json"), "w") as f:
        json.dump({"bits": BITS, "group_size": GROUP, "damp_percent": 0.01, "desc_act": desc_act, "static_groups": False, "sym": False,
                   "true_sequential": True, "model_name_or_path": None, "model_file_base_name": "model", "quant_method": "gptq",
                   "checkpoint_format": "gptq"}, f)


def load_checkpoint(path, seed=99):
    from safetensors.torch import load_file
    from autogptq_amd.model_utils import load_packed_layers

    with open(os.path.join(path, "quantize_config.json")) as f:
        qc = json.load(f)
    sd = load_file(os.path.join(path, "model.safetensors"))
    model = fresh_model(seed)
    return load_packed_layers(model, sd, qc["bits"], qc["group_size"], desc_act=qc["desc_act"], quant_method=qc["quant_method"],
                              checkpoint_format=qc["checkpoint_format"]), sd, qc


def make_twin(src_state, twin_w, seed=7):
    """fp16 Qwen2-MoE whose quantised weights are the dequantised ones and whose other tensors equal the quantised model's."""
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
