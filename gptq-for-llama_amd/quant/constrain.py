"""Constrained decoding for regular languages, host side: a deterministic automaton over TOKENS (TokenDFA) and the ways to get one -- a dense
table, a list of token sequences, a regular expression over the bytes of a vocabulary.  Plain numpy, no device; DecodeEngine.set_constraint
uploads the two tables and gptq_constrain_rows_f16 (csrc/constrain.hip; include/gptq_mi355x.h "constrained decoding") walks them per step.

The representation: a token v in state s leads to next[s, cls[v]]; -1 says the token is not allowed there.  Tokens whose columns are equal in
every state share a class, which shrinks the table from S x V to S x C -- C in the hundreds for a real vocabulary --, so grammars of thousands
of states fit.  The start state is 0.

The regex dialect of from_regex (matched over BYTES, exactly as Python's `re` matches a bytes pattern with re.fullmatch): literals and escaped
metacharacters; \\d \\D \\w \\W \\s \\S; \\n \\t \\r \\xHH; `.` (any byte but \\n); [...] with ranges, negation and class escapes; (...), (?:...) and |;
* + ? {m} {m,} {m,n} {,n}.  Anchors, back-references, look-around, lazy and possessive quantifiers, flags and named groups raise ValueError
naming the offset.

Not built yet: constraints under speculation and for beams, context-free grammars (they need a stack), the model.generate hook
(prefix_allowed_tokens_fn keeps going where it goes today), any tokenizer loading (llama_vocab_bytes takes the pieces as strings)."""
import re

import numpy as np

MAX_STATES = 32767          # GPTQ_CONSTRAIN_MAX_STATES
MAX_CLASSES = 16384         # GPTQ_CONSTRAIN_MAX_CLASSES
MAX_REPEAT = 4096           # {m,n} beyond this is refused: the expansion copies the operand


class TokenDFA:
    """an immutable deterministic automaton over token ids: n_states S, n_classes C, vocab V, cls int16 [V], next int16 [S, C], start state 0"""
    __slots__ = ('n_states', 'n_classes', 'vocab', 'cls', 'next')

    def __init__(self, cls, nxt):
        cls = np.ascontiguousarray(cls, dtype=np.int16)
        nxt = np.ascontiguousarray(nxt, dtype=np.int16)
        cls.setflags(write=False)
        nxt.setflags(write=False)
        for k, v in (('cls', cls), ('next', nxt), ('vocab', int(cls.shape[0])), ('n_states', int(nxt.shape[0])), ('n_classes', int(nxt.shape[1]))):
            object.__setattr__(self, k, v)

    def __setattr__(self, k, v):
        raise AttributeError('TokenDFA is immutable')

    def __repr__(self):
        return 'TokenDFA(states=%d, classes=%d, vocab=%d)' % (self.n_states, self.n_classes, self.vocab)

    # ---- helpers for tests and callers ----
    def allowed(self, state):
        """bool [V]: the tokens allowed in `state`"""
        return self.next[int(state)][self.cls] >= 0

    def step(self, state, token):
        """the state behind `token` in `state`, or -1"""
        state, token = int(state), int(token)
        if state < 0 or not 0 <= token < self.vocab:
            return -1
        return int(self.next[state, self.cls[token]])

    def walk(self, tokens, state=0):
        """the state after the token list from `state` (the start by default), or -1 as soon as a token is not allowed"""
        for t in tokens:
            state = self.step(state, t)
            if state < 0:
                return -1
        return state

    def dense(self):
        """the [S, V] table"""
        return self.next[:, self.cls]

    # ---- constructors ----
    @classmethod
    def from_table(cls, table, start=0):
        """table: dense int [S, V], table[s, v] = the state behind token v in state s, -1 for a banned token.  Keeps the states reachable from
        `start`, renumbers them (start -> 0, the others in their order) and compresses the classes.  ValueError for an entry outside [-1, S), a
        reachable state that allows no token (the kernel never sees a row it would empty), more than 32 767 states or 16 384 classes."""
        table = np.asarray(table)
        if table.ndim != 2 or table.shape[0] < 1 or table.shape[1] < 1 or table.dtype.kind not in 'iu':
            raise ValueError('TokenDFA.from_table: table must be an integer array [S >= 1, V >= 1]')
        return _from_columns('TokenDFA.from_table', table, None, start)

    @classmethod
    def from_sequences(cls, seqs, vocab, eos_token_id):
        """the language "exactly one of these token-id sequences, then eos" as a trie (the label-choice case).  ValueError for an empty list, an
        id outside [0, vocab), a sequence that holds eos itself."""
        what = 'TokenDFA.from_sequences'
        vocab, eos = int(vocab), int(eos_token_id)
        if vocab < 1 or not 0 <= eos < vocab:
            raise ValueError('%s: eos_token_id %d outside the vocabulary of %d' % (what, eos, vocab))
        seqs = [[int(t) for t in s] for s in seqs]
        if not seqs:
            raise ValueError('%s: no sequences' % what)
        children, accept = [{}], [False]
        for s in seqs:
            node = 0
            for t in s:
                if not 0 <= t < vocab or t == eos:
                    raise ValueError('%s: token %d is outside [0, %d) or is the eos token' % (what, t, vocab))
                if t not in children[node]:
                    children[node][t] = len(children)
                    children.append({})
                    accept.append(False)
                node = children[node][t]
            accept[node] = True
        n = len(children)
        if n + 1 > MAX_STATES:
            raise ValueError('%s: %d states, more than %d' % (what, n + 1, MAX_STATES))
        table = np.full((n + 1, vocab), -1, dtype=np.int32)
        for s, ch in enumerate(children):
            for t, c in ch.items():
                table[s, t] = c
            if accept[s]:
                table[s, eos] = n
        table[n, eos] = n                                          # FINAL allows only eos -> FINAL
        return _from_columns(what, table, None, 0)

    @classmethod
    def from_regex(cls, pattern, vocab_bytes, eos_token_id, max_states=4096):
        """the language "a token sequence whose bytes fully match `pattern`, then eos".  vocab_bytes: V bytes objects, the text of every token; None
        or b'' -- and the eos token itself -- never count as text.  Thompson NFA, subset construction to a byte DFA, token transitions by walking
        every token's bytes from every state (one numpy gather per byte position), accepting states get eos -> FINAL, FINAL allows only eos ->
        FINAL, transitions into states that cannot reach FINAL become -1 (generation never reaches a dead end), then from_table's steps.
        ValueError for what the dialect does not have (naming the offset), for a byte DFA or an automaton of more than max_states states, and for
        an empty language -- also one that this vocabulary cannot spell."""
        what = 'TokenDFA.from_regex'
        if not isinstance(pattern, str):
            raise ValueError('%s: pattern must be a str' % what)
        V, eos = len(vocab_bytes), int(eos_token_id)
        if V < 1 or not 0 <= eos < V:
            raise ValueError('%s: eos_token_id %d outside the vocabulary of %d' % (what, eos, V))
        max_states = int(max_states)
        trans, accept = regex_byte_dfa(pattern, max_states)
        Sb = trans.shape[0]
        # the distinct texts: tokens of equal bytes have equal columns.  Column U is "never allowed", column U + 1 the eos token
        texts, col_of = {}, np.empty(V, dtype=np.int64)
        for v, t in enumerate(vocab_bytes):
            if v == eos or t is None or len(t) == 0:
                col_of[v] = -1
                continue
            if not isinstance(t, (bytes, bytearray)):
                raise ValueError('%s: vocab_bytes[%d] must be bytes or None, not %r' % (what, v, type(t).__name__))
            col_of[v] = texts.setdefault(bytes(t), len(texts))
        U = len(texts)
        col_of[col_of < 0] = U
        col_of[eos] = U + 1
        FINAL = Sb
        table = np.full((Sb + 1, U + 2), -1, dtype=np.int32)
        table[:Sb, :U] = _token_transitions(trans, list(texts))
        table[:Sb, U + 1] = np.where(accept, FINAL, -1)
        table[FINAL, U + 1] = FINAL
        # states that reach FINAL, backwards over the distinct edges
        succ = [np.unique(row[row >= 0]) for row in table]
        pred = [[] for _ in range(Sb + 1)]
        for s, ts in enumerate(succ):
            for t in ts.tolist():
                pred[t].append(s)
        good = np.zeros(Sb + 2, dtype=bool)                        # (the last entry stands for -1)
        good[FINAL] = True
        stack = [FINAL]
        while stack:
            for s in pred[stack.pop()]:
                if not good[s]:
                    good[s] = True
                    stack.append(s)
        if not good[0]:
            raise ValueError('%s: the language is empty (no token sequence of this vocabulary fully matches %r)' % (what, pattern))
        table[~good[table]] = -1
        dfa = _from_columns(what, table, col_of, 0)
        if dfa.n_states > max_states:
            raise ValueError('%s: %d states, more than max_states = %d' % (what, dfa.n_states, max_states))
        return dfa


def _from_columns(what, table, col_of, start):
    """from_table's steps on a table of DISTINCT columns [S, U] with token v in column col_of[v] (None: the identity)"""
    S = table.shape[0]
    start = int(start)
    if not 0 <= start < S:
        raise ValueError('%s: start %d outside [0, %d)' % (what, start, S))
    if int(table.min()) < -1 or int(table.max()) >= S:
        raise ValueError('%s: an entry lies outside [-1, %d)' % (what, S))
    reach = np.zeros(S, dtype=bool)
    reach[start] = True
    stack = [start]
    while stack:
        row = table[stack.pop()]
        for t in np.unique(row[row >= 0]).tolist():
            if not reach[t]:
                reach[t] = True
                stack.append(t)
    order = [start] + [s for s in np.flatnonzero(reach).tolist() if s != start]
    if len(order) > MAX_STATES:
        raise ValueError('%s: %d reachable states, more than %d' % (what, len(order), MAX_STATES))
    new_id = np.full(S + 1, -1, dtype=np.int32)                    # (the last entry maps -1 to -1)
    new_id[order] = np.arange(len(order), dtype=np.int32)
    table = new_id[table[order]]
    used = table if col_of is None else table[:, np.unique(col_of)]
    empty = np.flatnonzero(~(used >= 0).any(axis=1))
    if empty.size:
        raise ValueError('%s: reachable state %d allows no token' % (what, order[int(empty[0])]))
    # classes: the distinct columns
    cols = np.ascontiguousarray(table.T.astype(np.int16))
    keys = cols.view(np.dtype((np.void, cols.shape[1] * 2))).ravel()
    _, first, inverse = np.unique(keys, return_index=True, return_inverse=True)
    if first.size > MAX_CLASSES:
        raise ValueError('%s: %d classes, more than %d' % (what, first.size, MAX_CLASSES))
    inverse = inverse.ravel()
    return TokenDFA(inverse if col_of is None else inverse[col_of], cols[first].T)


def _token_transitions(trans, texts):
    """[Sb, U] int32: the byte DFA's state behind text u from state s, -1 where it dies.  Vectorised over [states, texts], one gather per byte
    position, in blocks of states that bound the temporaries"""
    Sb, U = trans.shape[0], len(texts)
    out = np.empty((Sb, U), dtype=np.int32)
    if U == 0:
        return out
    lens = np.array([len(t) for t in texts], dtype=np.int64)
    L = int(lens.max())
    padded = np.zeros((U, L), dtype=np.int64)
    for u, t in enumerate(texts):
        padded[u, :len(t)] = np.frombuffer(t, dtype=np.uint8)
    ext = np.vstack([np.where(trans < 0, Sb, trans), np.full((1, 256), Sb, dtype=trans.dtype)]).astype(np.int32)      # row Sb: the dead state
    block = max(1, (1 << 22) // U)
    for s0 in range(0, Sb, block):
        cur = np.repeat(np.arange(s0, min(Sb, s0 + block), dtype=np.int32)[:, None], U, axis=1)
        for p in range(L):
            live = lens > p
            cur[:, live] = ext[cur[:, live], padded[live, p][None, :]]
        out[s0:s0 + block] = np.where(cur == Sb, -1, cur)
    return out


# ---- the regex: parser -> Thompson NFA -> byte DFA ------------------------------------------------------------------------------------------
def _mask(codes):
    m = np.zeros(256, dtype=bool)
    m[list(codes)] = True
    return m


_DIGIT = _mask(range(48, 58))
_WORD = _mask(list(range(48, 58)) + list(range(65, 91)) + list(range(97, 123)) + [95])
_SPACE = _mask([9, 10, 11, 12, 13, 32])
_CLASS_ESCAPES = {ord('d'): _DIGIT, ord('D'): ~_DIGIT, ord('w'): _WORD, ord('W'): ~_WORD, ord('s'): _SPACE, ord('S'): ~_SPACE}
_CHAR_ESCAPES = {ord('n'): 10, ord('t'): 9, ord('r'): 13}
_QUANT = re.compile(rb'\{(\d*)(?:(,)(\d*))?\}')


class _Parser:
    """pattern bytes -> a tree of ('set', mask) / ('cat', [nodes]) / ('alt', [nodes]) / ('rep', node, m, n or None)"""

    def __init__(self, pat):
        self.pat, self.p = pat, 0

    def error(self, msg, at=None):
        return ValueError('regex: %s at offset %d of %r' % (msg, self.p if at is None else at, self.pat))

    def peek(self):
        return self.pat[self.p] if self.p < len(self.pat) else None

    def parse(self):
        node = self.alt()
        if self.p < len(self.pat):
            raise self.error('unbalanced )')
        return node

    def alt(self):
        branches = [self.cat()]
        while self.peek() == ord('|'):
            self.p += 1
            branches.append(self.cat())
        return branches[0] if len(branches) == 1 else ('alt', branches)

    def cat(self):
        items = []
        while self.peek() is not None and self.peek() not in b'|)':
            items.append(self.repeat())
        return items[0] if len(items) == 1 else ('cat', items)

    def quantifier(self):
        """(m, n or None, length) of the quantifier at p, or None"""
        c = self.peek()
        if c == ord('*'):
            return 0, None, 1
        if c == ord('+'):
            return 1, None, 1
        if c == ord('?'):
            return 0, 1, 1
        if c == ord('{'):
            m = _QUANT.match(self.pat, self.p)
            if m is None or (m.group(2) is None and not m.group(1)):
                return None                                        # (as in `re`: a brace that opens no quantifier is a literal)
            lo = int(m.group(1)) if m.group(1) else 0
            hi = lo if m.group(2) is None else (int(m.group(3)) if m.group(3) else None)
            if hi is not None and hi < lo:
                raise self.error('min repeat greater than max repeat')
            if lo > MAX_REPEAT or (hi is not None and hi > MAX_REPEAT):
                raise self.error('a repeat count above %d' % MAX_REPEAT)
            return lo, hi, m.end() - m.start()
        return None

    def repeat(self):
        if self.quantifier() is not None:
            raise self.error('nothing to repeat')
        node = self.atom()
        q = self.quantifier()
        if q is not None:
            self.p += q[2]
            c = self.peek()
            if c == ord('?'):
                raise self.error('lazy quantifiers are not supported')
            if c == ord('+'):
                raise self.error('possessive quantifiers are not supported')
            if self.quantifier() is not None:
                raise self.error('multiple repeat')
            node = ('rep', node, q[0], q[1])
        return node

    def atom(self):
        c, at = self.peek(), self.p
        self.p += 1
        if c == ord('('):
            if self.peek() == ord('?'):
                if self.pat[self.p:self.p + 2] != b'?:':
                    raise self.error('flags, look-around and named groups are not supported', at)
                self.p += 2
            node = self.alt()
            if self.peek() != ord(')'):
                raise self.error('missing )', at)
            self.p += 1
            return node
        if c == ord('['):
            return ('set', self.char_class(at))
        if c == ord('.'):
            return ('set', ~_mask([10]))
        if c in b'^$':
            raise self.error('anchors are not supported (the whole text is matched)', at)
        if c == ord('\\'):
            e = self.escape(at, False)
            return ('set', e if isinstance(e, np.ndarray) else _mask([e]))
        return ('set', _mask([c]))

    def escape(self, at, in_class):
        """behind a backslash: a byte code or a class mask"""
        c = self.peek()
        if c is None:
            raise self.error('bad escape (end of pattern)', at)
        self.p += 1
        if c in _CLASS_ESCAPES:
            return _CLASS_ESCAPES[c]
        if c in _CHAR_ESCAPES:
            return _CHAR_ESCAPES[c]
        if c == ord('x'):
            h = self.pat[self.p:self.p + 2]
            if len(h) != 2 or not re.fullmatch(rb'[0-9a-fA-F]{2}', h):
                raise self.error('incomplete escape \\x', at)
            self.p += 2
            return int(h, 16)
        if ord('1') <= c <= ord('9') and not in_class:
            raise self.error('back-references are not supported', at)
        if c in b'AZbB' and not in_class:
            raise self.error('anchors are not supported (the whole text is matched)', at)
        if c < 128 and chr(c).isalnum():
            raise self.error('unsupported escape \\%s' % chr(c), at)
        return c                                                   # an escaped metacharacter (any other byte: itself)

    def char_class(self, at):
        m = np.zeros(256, dtype=bool)
        negate = self.peek() == ord('^')
        if negate:
            self.p += 1
        first = True
        while True:
            c = self.peek()
            if c is None:
                raise self.error('unterminated character set', at)
            if c == ord(']') and not first:
                self.p += 1
                break
            first = False
            lo_at = self.p
            lo = self.class_item()
            if self.peek() == ord('-') and self.p + 1 < len(self.pat) and self.pat[self.p + 1] != ord(']'):
                self.p += 1
                hi = self.class_item()
                if isinstance(lo, np.ndarray) or isinstance(hi, np.ndarray) or hi < lo:
                    raise self.error('bad character range', lo_at)
                m[lo:hi + 1] = True
            elif isinstance(lo, np.ndarray):
                m |= lo
            else:
                m[lo] = True
        return ~m if negate else m

    def class_item(self):
        c, at = self.peek(), self.p
        if c is None:
            raise self.error('unterminated character set', at)
        self.p += 1
        return self.escape(at, True) if c == ord('\\') else c


class _NFA:
    def __init__(self):
        self.eps, self.edges = [], []                              # per state: epsilon targets, (mask index, target) pairs
        self.masks, self._mask_ids = [], {}

    def state(self):
        self.eps.append([])
        self.edges.append([])
        return len(self.eps) - 1

    def mask_id(self, m):
        k = m.tobytes()
        if k not in self._mask_ids:
            self._mask_ids[k] = len(self.masks)
            self.masks.append(m)
        return self._mask_ids[k]

    def build(self, node):
        """Thompson: (start, end) of the fragment"""
        kind = node[0]
        if kind == 'set':
            s, e = self.state(), self.state()
            self.edges[s].append((self.mask_id(node[1]), e))
            return s, e
        if kind == 'cat':
            s = e = self.state()
            for item in node[1]:
                a, b = self.build(item)
                self.eps[e].append(a)
                e = b
            return s, e
        if kind == 'alt':
            s, e = self.state(), self.state()
            for item in node[1]:
                a, b = self.build(item)
                self.eps[s].append(a)
                self.eps[b].append(e)
            return s, e
        _, item, lo, hi = node
        s = e = self.state()
        for _ in range(lo):
            a, b = self.build(item)
            self.eps[e].append(a)
            e = b
        if hi is None:                                             # a star behind the lo copies
            a, b = self.build(item)
            end = self.state()
            self.eps[e] += [a, end]
            self.eps[b] += [a, end]
            return s, end
        end = self.state()
        for _ in range(hi - lo):                                   # optional copies: each may be skipped to the end
            a, b = self.build(item)
            self.eps[e] += [a, end]
            e = b
        self.eps[e].append(end)
        return s, end


def regex_byte_dfa(pattern, max_states=4096):
    """pattern (a str, matched over its UTF-8 bytes) -> (trans int32 [S, 256] with -1 for "no match possible", accept bool [S]), start state 0:
    the DFA accepts exactly the byte strings re.fullmatch(pattern.encode(), s) accepts.  ValueError for what the dialect lacks, for more than
    max_states states and for an empty language."""
    tree = _Parser(pattern.encode('utf-8')).parse()
    nfa = _NFA()
    start, end = nfa.build(tree)
    # bytes that no set of the pattern tells apart move alike: one representative per group
    member = np.stack(nfa.masks) if nfa.masks else np.zeros((1, 256), dtype=bool)
    _, byte_group = np.unique(member.T, axis=0, return_inverse=True)
    byte_group = byte_group.ravel()
    G = int(byte_group.max()) + 1
    rep = np.array([int(np.flatnonzero(byte_group == g)[0]) for g in range(G)])
    in_group = member[:, rep]                                      # [masks, groups]

    def closure(states):
        seen, stack = set(states), list(states)
        while stack:
            for t in nfa.eps[stack.pop()]:
                if t not in seen:
                    seen.add(t)
                    stack.append(t)
        return frozenset(seen)

    first = closure([start])
    ids, todo, rows = {first: 0}, [first], []
    while todo:
        cur = todo.pop()
        row = np.full(G, -1, dtype=np.int32)
        edges = [(mid, t) for q in cur for mid, t in nfa.edges[q]]
        for g in range(G):
            tgt = [t for mid, t in edges if in_group[mid, g]]
            if not tgt:
                continue
            nxt = closure(tgt)
            if nxt not in ids:
                if len(ids) >= max_states:
                    raise ValueError('regex: the byte DFA of %r has more than max_states = %d states' % (pattern, max_states))
                ids[nxt] = len(ids)
                todo.append(nxt)
            row[g] = ids[nxt]
        rows.append((ids[cur], row))
    S = len(ids)
    trans_g = np.empty((S, G), dtype=np.int32)
    for i, row in rows:
        trans_g[i] = row
    accept = np.zeros(S, dtype=bool)
    for st, i in ids.items():
        accept[i] = end in st
    # states that cannot reach an accepting one are dead: -1
    alive = accept.copy()
    changed = True
    while changed:
        ext = np.append(alive, False)
        now = alive | ext[trans_g].any(axis=1)
        changed = bool((now != alive).any())
        alive = now
    if not alive[0]:
        raise ValueError('regex: the language of %r is empty' % pattern)
    trans_g[~np.append(alive, False)[trans_g]] = -1
    return trans_g[:, byte_group], accept


def llama_vocab_bytes(pieces, special_ids=()):
    """the bytes of every token of a sentencepiece (Llama) vocabulary from its piece strings, for from_regex: U+2581 becomes a space, a byte
    piece <0xNN> becomes that byte, the ids in special_ids (and pieces that are None) become None -- never allowed.  A pure function: no
    tokenizer is loaded."""
    special = set(int(i) for i in special_ids)
    out = []
    for i, p in enumerate(pieces):
        if i in special or p is None:
            out.append(None)
            continue
        m = re.fullmatch(r'<0x([0-9A-Fa-f]{2})>', p)
        out.append(bytes([int(m.group(1), 16)]) if m else p.replace('▁', ' ').encode('utf-8'))
    return out
