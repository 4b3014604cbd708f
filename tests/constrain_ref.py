"""numpy restatement of gptq_constrain_rows_f16 (include/gptq_mi355x.h "constrained decoding"), rule by rule in the header's order.  It works on
the BITS of the fp16 logits (uint16 views), so NaN payloads, +-inf and -0.0 pass through untouched exactly where the kernel must leave them.
Shared by tests/test_host_constrain.py (pinned there to transformers' PrefixConstrainedLogitsProcessor) and the GPU tests, whose oracle it is."""
import numpy as np

MAX_SEQS, MAX_STATES, MAX_CLASSES = 65535, 32767, 16384
NEG_INF = 0xFC00


def constrain_rows(logits, vocab, nxt, n_states, n_classes, cls, map_of, state, last, lens, len_add, t_limit):
    """logits fp16 [B, ld] (ld >= vocab: the padding is never touched), nxt int16 [>= n_states, ld_next >= n_classes], cls int16
    [n_maps, ld_cls >= vocab], map_of int32 [B], state int32 [B], last int64 [B] or None, lens int64 [B].  Returns (new logits, new state)."""
    bits = np.array(np.asarray(logits, dtype=np.float16).view(np.uint16), copy=True)
    state = np.array(state, dtype=np.int32, copy=True)
    nxt, cls = np.asarray(nxt, dtype=np.int16), np.asarray(cls, dtype=np.int16)
    n_maps = cls.shape[0]
    for b in range(bits.shape[0]):
        nb = int(lens[b]) + int(len_add)
        if nb < 0 or nb > t_limit:                                  # 1 idle
            continue
        s = int(state[b])
        if s < 0:                                                   # 2 switched off
            continue
        m = int(map_of[b])
        s2 = s
        if s >= n_states or not 0 <= m < n_maps:                    # 4 a state or a map that is not in the tables
            s2 = -2
        elif last is not None:                                      # 3 advance
            t = int(last[b])
            s2 = -2
            if 0 <= t < vocab:
                c = int(cls[m, t])
                if 0 <= c < n_classes:
                    e = int(nxt[s, c])
                    if 0 <= e < n_states:
                        s2 = e
        if last is not None or s2 != s:                             # 5, 6
            state[b] = s2
        if s2 < 0:                                                  # 4 left: the row keeps its bits
            continue
        c = cls[m, :vocab].astype(np.int64)                         # 7 mask
        ok = (c >= 0) & (c < n_classes)
        e = nxt[s2].astype(np.int64)[np.where(ok, c, 0)]
        ok &= (e >= 0) & (e < n_states)
        bits[b, :vocab][~ok] = NEG_INF
    return bits.view(np.float16), state


def constrain_dfa(logits, dfa, state, last=None):
    """the same rules for rows that all run under ONE TokenDFA, with no idle row: (new logits [B, V], new state)"""
    logits = np.asarray(logits, dtype=np.float16)
    B = logits.shape[0]
    return constrain_rows(logits, dfa.vocab, dfa.next, dfa.n_states, dfa.n_classes, dfa.cls[None], np.zeros(B, dtype=np.int32), state, last,
                          np.zeros(B, dtype=np.int64), 0, 0)
