"""Randomly initialised tiny models with UNGATED MLPs, act(fc1(x) + b) -- OPT (ReLU), Phi (gelu_new = tanh-GELU) and GPT-NeoX (erf GELU): 2 blocks, hidden 256,
ffn 1024, biases -- quantised and packed the way _tiny_llama does it for the tiny Llama (the oracle's min/max quantizer, this backend's pack_model).  A plain
helper module like _tiny_gemma.py."""
import torch

from oracle import gptq_oracle as O

BITS, GROUP = 4, 64
BLOCKS = {"opt": "model.decoder.layers.", "phi": "model.layers.", "neox": "gpt_neox.layers."}


def fresh_model(kind, seed):
    torch.manual_seed(seed)
    if kind == "opt":
        from transformers import OPTConfig, OPTForCausalLM
        m = OPTForCausalLM(OPTConfig(hidden_size=256, ffn_dim=1024, num_hidden_layers=2, num_attention_heads=4, vocab_size=512, max_position_embeddings=128,
                                     word_embed_proj_dim=256, activation_function="relu", enable_bias=True, dropout=0.0, attn_implementation="eager",
                                     tie_word_embeddings=False, pad_token_id=1, bos_token_id=2, eos_token_id=2))
    elif kind == "phi":
        from transformers import PhiConfig, PhiForCausalLM
        m = PhiForCausalLM(PhiConfig(hidden_size=256, intermediate_size=1024, num_hidden_layers=2, num_attention_heads=4, vocab_size=512,
                                     max_position_embeddings=128, hidden_act="gelu_new", resid_pdrop=0.0, embd_pdrop=0.0, attn_implementation="eager",
                                     tie_word_embeddings=False, pad_token_id=1, bos_token_id=2, eos_token_id=2))
    else:
        from transformers import GPTNeoXConfig, GPTNeoXForCausalLM
        m = GPTNeoXForCausalLM(GPTNeoXConfig(hidden_size=256, intermediate_size=1024, num_hidden_layers=2, num_attention_heads=4, vocab_size=512,
                                             max_position_embeddings=128, hidden_act="gelu", hidden_dropout=0.0, attention_dropout=0.0,
                                             attn_implementation="eager", tie_word_embeddings=False, pad_token_id=1, bos_token_id=2, eos_token_id=2))
    head = m.get_output_embeddings()
    head.weight.data.normal_(0, 0.3)               # spread the logits, as the tiny Llama does
    m.tiny_kind = kind
    return m.half().eval()


def quantizable(model):
    from autogptq_amd.model_utils import find_layers
    prefix = BLOCKS[model.tiny_kind]
    return {n: l for n, l in find_layers(model).items() if n.startswith(prefix)}


def quantize_and_pack(model):
    """Oracle min/max quantizer per (group, column) -> quantizers dict -> pack_model on the linears of the decoder blocks.  The first linear of every MLP is
    scaled up first (pre-activations beyond 1: off the activation's linear part)."""
    from autogptq_amd.fused import PLAIN_ACT_SITES
    from autogptq_amd.model_utils import pack_model
    for mod in model.modules():
        site = PLAIN_ACT_SITES.get(type(mod).__name__)
        if site is not None:
            getattr(mod, site[0]).weight.data.mul_(4.0)
    quantizers = {}
    for name, lin in quantizable(model).items():
        gi = torch.from_numpy(O.default_g_idx(lin.in_features, GROUP))
        s, z = O.minmax_quantize(lin.weight.data.float(), BITS, GROUP, g_idx=gi.numpy())
        quantizers[name] = (None, s.half(), z.half(), gi)
    pack_model(model, quantizers, BITS, GROUP)
    return quantizers
