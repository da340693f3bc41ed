"""Shared by the CPU and GPU mixture-of-experts tests: a randomly initialised tiny Mixtral (transformers 5 layout: 3-D expert parameters), its attention
linears and experts quantised with the oracle's min/max quantizer, packed (pack_model + pack_moe_experts), saved with AutoGPTQ's Mixtral names
(``block_sparse_moe.experts.{e}.w1 / w3 / w2``), and its dequantised fp16 twin."""
import json
import os

import torch

from oracle import gptq_oracle as O

BITS, GROUP = 4, 64
H, I, E, TOPK = 256, 512, 8, 2


def tiny_config():
    from transformers import MixtralConfig
    return MixtralConfig(hidden_size=H, intermediate_size=I, num_hidden_layers=2, num_attention_heads=4, num_key_value_heads=4, num_local_experts=E,
                         num_experts_per_tok=TOPK, vocab_size=512, max_position_embeddings=128, attn_implementation="sdpa", tie_word_embeddings=False)


def fresh_model(seed):
    from transformers import MixtralForCausalLM
    torch.manual_seed(seed)
    m = MixtralForCausalLM(tiny_config())
    m.lm_head.weight.data.normal_(0, 0.3)
    for mod in m.modules():                        # transformers leaves the 3-D expert parameters uninitialised: give them a scale like the linears'
        if hasattr(mod, "gate_up_proj") and torch.is_tensor(mod.gate_up_proj):
            mod.gate_up_proj.data.normal_(0, 0.05)
            mod.down_proj.data.normal_(0, 0.05)
    return m.half().eval()


def _quant(W, desc_act, gen):
    """[N, K] weight -> (None, scale, zero, g_idx) as pack_model takes them."""
    K = W.shape[1]
    gi = torch.from_numpy(O.default_g_idx(K, GROUP))
    if desc_act:
        gi = gi[torch.randperm(K, generator=gen)].contiguous()
    s, z = O.minmax_quantize(W.float(), BITS, GROUP, g_idx=gi.numpy())
    return (None, s.half(), z.half(), gi)


def quantize_and_pack(model, desc_act, seed=0):
    """Attention linears through pack_model, experts through pack_moe_experts.  Returns the twin's weights {state-dict key: dequantised tensor}
    computed by the ORACLE from the packed tensors (linears: [N, K]; experts: the 3-D gate_up_proj / down_proj)."""
    from autogptq_amd.model_utils import find_layers, pack_model
    from autogptq_amd.moe import dense_expert_modules, pack_moe_experts

    gen = torch.Generator().manual_seed(seed)
    lin = {n: l for n, l in find_layers(model).items() if n.startswith("model.layers.") and ".self_attn." in n}
    quantizers = {n: _quant(l.weight.data, desc_act, gen) for n, l in lin.items()}
    ex_q = {}
    dense = dense_expert_modules(model)
    for path, m in dense.items():
        for e in range(m.num_experts):
            gu, dn = m.gate_up_proj.data[e], m.down_proj.data[e]
            for nm, W in (("w1", gu[:I]), ("w3", gu[I:]), ("w2", dn)):
                ex_q[f"{path}.{e}.{nm}"] = _quant(W, desc_act, gen)
    pack_model(model, quantizers, BITS, GROUP, desc_act=desc_act)
    pack_moe_experts(model, ex_q, BITS, GROUP, desc_act=desc_act)
    mode = O.reference_zero_mode(desc_act, BITS)

    def dq(q):
        return O.dequantize(q.qweight.cpu(), q.qzeros.cpu(), q.scales.cpu(), q.g_idx.cpu(), BITS, mode)      # [K, N]

    twin_w = {n + ".weight": dq(model.get_submodule(n)).t().contiguous() for n in quantizers}
    for path in dense:
        q = model.get_submodule(path)
        twin_w[path + ".gate_up_proj"] = torch.stack([torch.cat([dq(q[e].w1).t(), dq(q[e].w3).t()], 0) for e in range(E)]).contiguous()
        twin_w[path + ".down_proj"] = torch.stack([dq(q[e].w2).t() for e in range(E)]).contiguous()
    return twin_w


def autogptq_names(sd):
    """The state dict as AutoGPTQ saves a Mixtral: the MoE block under ``block_sparse_moe``."""
    return {k.replace(".mlp.", ".block_sparse_moe."): v for k, v in sd.items()}


def save_checkpoint(model, path, desc_act):
    from safetensors.torch import save_file
    os.makedirs(path, exist_ok=True)
    sd = autogptq_names({k: v.detach().cpu().contiguous() for k, v in model.state_dict().items()})
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
    """fp16 Mixtral whose quantised weights are the dequantised ones and whose other tensors equal the quantised model's."""
    twin = fresh_model(seed)
    sd = twin.state_dict()
    for k in sd:
        if k in src_state and src_state[k].shape == sd[k].shape and src_state[k].dtype == sd[k].dtype:
            sd[k] = src_state[k].clone()
    for k, W in twin_w.items():
        sd[k] = W.to(sd[k].dtype).clone()
    twin.load_state_dict(sd)
    return twin
