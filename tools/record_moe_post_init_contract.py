"""Record what ``QuantMoEExperts.post_init`` settles, switch set by switch set: tests/golden/moe_post_init_contract.json, the fixture of
tests/test_gpu_moe_post_init_contract.py (which imports the cases and ``observe`` from here, so recorder and test cannot drift apart).

    timeout 900 python tools/record_moe_post_init_contract.py          # needs the GPU; rewrites the fixture from whatever revision is checked out

Record only from a revision whose answers are meant to be the contract (the fixture in the tree: the revision before post_init was restructured around
one table of the routed copy paths), and review the JSON diff.

Cases, per width (2, 3, 4, 8 bits) on E = 2, top_k = 2, H = 256, I = 512, fp16 experts with random packed weights from a fixed seed:

* "main"   g128: every combination of the seven switches (the keywords decode_copy, batch, prefill, low_bit, low_bit_decode, the attributes low_bit_batch,
           low_bit_prefill); backward=True on four of them (nothing, all 4/8-bit switches, all low-bit switches, everything);
* "rows"   one oddity at a time (ROWS: group sizes, sizes, dtypes, top_k; H = 65536 is the row whose decline only the decode plan finds, after the
           copies were built) x nine switch sets (each switch alone, all 4/8-bit switches, all low-bit switches);
* "tune"   3- and 4-bit, everything on: the four ``*_tokens`` tunables moved (TUNABLES).

Per case, after post_init and once more after ``_invalidate()`` + ``_ensure_init()`` (a move, a state-dict load): the warnings of the autogptq_amd.moe logger,
the two switch attributes, decode_copy_bytes, which tables exist, the flags of the struct each entry point gets, whether the layers hold a decode copy,
plan(T) path / reason and workspace_bytes(T) at T in TS, backward_workspace_bytes(300), and the scratch autogptq_post_init reserves for the module at
max_input_length in LENGTHS.  A post_init that raises is recorded by its exception.

The file is kept small by tables: "states" and "warnings" hold each distinct answer once, "cases" maps a case name to
[warnings, state, warnings after re-initialisation, state after re-initialisation] as indices."""
import itertools
import json
import logging
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from autogptq_amd.moe import QuantMoEExperts  # noqa: E402

FIXTURE = os.path.join(ROOT, "tests", "golden", "moe_post_init_contract.json")
BITS = (2, 3, 4, 8)
E, TOPK, H, I = 2, 2, 256, 512
SWITCHES = ("decode_copy", "batch", "prefill", "low_bit", "low_bit_decode", "low_bit_batch", "low_bit_prefill")      # the last two are attributes
ATTRIBUTES = ("low_bit_batch", "low_bit_prefill")
WIDE = ("decode_copy", "batch", "prefill")                                        # the 4/8-bit switches
LOW = ("low_bit", "low_bit_decode", "low_bit_batch", "low_bit_prefill")           # the low-bit switches
TS = (1, 4, 5, 64, 65, 300)
LENGTHS = (3, 40, 300)
DEFAULT_TUNABLES = dict(batch_max_tokens=64, low_bit_batch_max_tokens=64, low_bit_prefill_min_tokens=65, low_bit_decode_max_tokens=4)
# the decline rows: name -> what differs from (gs=128, H, I, fp16, top_k=2)
ROWS = {
    "g32": dict(gs=32), "g64": dict(gs=64), "g-1": dict(gs=-1), "g48": dict(gs=48), "I192": dict(I=192), "H192": dict(H=192),
    "f32": dict(dtype=torch.float32), "topk9": dict(top_k=9), "bf16": dict(dtype=torch.bfloat16),
    "H65536": dict(H=65536),      # the one row whose decline the metadata does not show: the decode plan's staged row does not fit the LDS, the batch and prefill plans accept
}
TUNABLES = {
    "bmax16": dict(batch_max_tokens=16), "lbmax16": dict(low_bit_batch_max_tokens=16), "ldmax2": dict(low_bit_decode_max_tokens=2),
    "lpmin1": dict(low_bit_prefill_min_tokens=1), "lpmin200": dict(low_bit_prefill_min_tokens=200),
}


def _name(on):
    return "+".join(s for s in SWITCHES + ("backward",) if s in on) or "none"


def cases(bits):
    """[(case name, row name, switches that are on, tunables)] of one width, in a fixed order."""
    out = []
    for r in range(len(SWITCHES) + 1):
        for on in itertools.combinations(SWITCHES, r):
            out.append((f"main/{_name(on)}", "g128", on, {}))
    for on in ((), WIDE, LOW, SWITCHES):
        out.append((f"main/{_name(on + ('backward',))}", "g128", on + ("backward",), {}))
    for row in ROWS:
        for on in [(s,) for s in SWITCHES] + [WIDE, LOW]:
            out.append((f"{row}/{_name(on)}", row, on, {}))
    if bits in (3, 4):
        for tname, tun in TUNABLES.items():
            out.append((f"tune/{tname}", "g128", SWITCHES, tun))
    return out


def make_experts(bits, row, dev):
    """The experts of one row on the device, not post-initialised (random packed weights; seed: bits and row)."""
    kw = dict(gs=128, H=H, I=I, dtype=torch.float16, top_k=TOPK)
    kw.update(ROWS.get(row, {}))
    gen = torch.Generator().manual_seed(1000 * bits + sorted(["g128", *ROWS]).index(row))
    q = QuantMoEExperts(E, kw["H"], kw["I"], bits, kw["gs"], top_k=kw["top_k"], weight_dtype=kw["dtype"])
    for e in range(E):
        for lin in q[e].layers():
            lin.qweight = torch.randint(-2 ** 31, 2 ** 31 - 1, lin.qweight.shape, generator=gen, dtype=torch.int64).to(torch.int32)
            lin.qzeros = torch.randint(-2 ** 31, 2 ** 31 - 1, lin.qzeros.shape, generator=gen, dtype=torch.int64).to(torch.int32)
            lin.scales = (torch.rand(lin.scales.shape, generator=gen) * 0.004 + 0.001).to(lin.scales.dtype)
    return q.to(dev)


def recorded_token_counts(q, rows, on):
    """The token counts at which the recorded revision's autogptq_post_init asked workspace_bytes: assembled there from the caller's expert_* keywords."""
    ts = {rows, *range(1, min(rows, 4) + 1)}
    if "batch" in on:
        ts.add(min(rows, q.batch_max_tokens))
    if "low_bit_batch" in on and q.bits in (2, 3):
        ts.add(min(rows, 64, int(q.low_bit_batch_max_tokens)))
    if "prefill" in on:
        ts.add(min(rows, 64))
    if "low_bit_prefill" in on and q.bits in (2, 3):
        ts.add(min(rows, max(64, int(q.low_bit_prefill_min_tokens) - 1)))
    return sorted(ts)


class _Capture(logging.Handler):
    def __init__(self):
        super().__init__(logging.WARNING)
        self.messages = []

    def emit(self, record):
        self.messages.append(record.getMessage())


def _state(q, on, token_counts):
    def copies():
        held = [lin._qweight_tiled is not None for e in range(q.num_experts) for lin in q[e].layers()]
        return "all" if all(held) else "none" if not any(held) else "mixed"

    def reserved(rows):
        need = max(q.workspace_bytes(t, q.top_k) for t in token_counts(q, rows, on))
        return max(need, q.backward_workspace_bytes(rows, q.top_k)) if q._grad_table is not None else need

    plans = [q.plan(T) for T in TS]
    return {
        "low_bit_batch": q.low_bit_batch, "low_bit_prefill": q.low_bit_prefill, "decode_copy_bytes": q.decode_copy_bytes,
        "decode_table": q._decode_table is not None, "grad_table": q._grad_table is not None, "copies": copies(),
        "flags": [q._moe.flags, q._moe_of("batch").flags, q._moe_of("prefill").flags],
        "plans": [[p["path"], p["reason"], q.workspace_bytes(T)] for p, T in zip(plans, TS)],
        "backward_workspace_bytes": q.backward_workspace_bytes(300), "reserved": [reserved(rows) for rows in LENGTHS],
    }


def observe(q, on, tunables, token_counts):
    """[warnings, state, warnings, state] of one case on the experts ``q``: post_init with the switches ``on``, then a re-initialisation.
    ``token_counts(q, rows, on)``: the token counts whose workspace autogptq_post_init reserves."""
    q._invalidate()
    for name, value in {**DEFAULT_TUNABLES, **tunables}.items():
        setattr(q, name, value)
    for name in ATTRIBUTES:
        setattr(q, name, name in on)
    log, cap = logging.getLogger("autogptq_amd.moe"), _Capture()
    log.addHandler(cap)
    out = []
    try:
        for phase in (lambda: q.post_init(**{s: s in on for s in SWITCHES + ("backward",) if s not in ATTRIBUTES}),
                      lambda: (q._invalidate(), q._ensure_init())):
            cap.messages = []
            try:
                phase()
                state = _state(q, on, token_counts)
            except Exception as exc:        # (a layer set the library refuses outright: the case is its exception)
                state = {"raises": f"{type(exc).__name__}: {exc}"}
            out += [list(cap.messages), state]
    finally:
        log.removeHandler(cap)
    return out


def record(dev="cuda:0"):
    states, warnings, table, dropped, seconds = [], [], {}, [], {}

    def intern(pool, item):
        key = json.dumps(item, sort_keys=True)
        if key not in pool:
            pool.append(key)
        return pool.index(key)

    for bits in BITS:
        t0, built = time.perf_counter(), {}
        for name, row, on, tun in cases(bits):
            if row not in built:
                try:
                    built[row] = make_experts(bits, row, dev)
                except Exception as exc:
                    built[row] = None
                    dropped.append(f"{bits}-bit {row}: {type(exc).__name__}: {exc}")
            if built[row] is None:
                continue
            w1, s1, w2, s2 = observe(built[row], on, tun, recorded_token_counts)
            table[f"{bits}/{name}"] = [intern(warnings, w1), intern(states, s1), intern(warnings, w2), intern(states, s2)]
        torch.cuda.synchronize()
        seconds[bits] = round(time.perf_counter() - t0, 1)
        print(f"{bits}-bit: {len([k for k in table if k.startswith(f'{bits}/')])} cases in {seconds[bits]} s", flush=True)
    doc = {"dropped_rows": dropped, "warnings": [json.loads(s) for s in warnings], "states": [json.loads(s) for s in states], "cases": table}
    with open(FIXTURE, "w") as f:
        json.dump(doc, f, separators=(",", ":"), sort_keys=True)
        f.write("\n")
    print(f"{len(table)} cases, {len(states)} states, {len(warnings)} warning lists, {os.path.getsize(FIXTURE)} bytes -> {FIXTURE}")
    return seconds


if __name__ == "__main__":
    record()
