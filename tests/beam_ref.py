"""The float64 restatement of the beam-search rule of include/gptq_mi355x.h "beam search" (HF's `_beam_search` for one prompt, do_sample=False, at
most one EOS id, no logit processors): one step on N rows of logits (step), the whole search on a function that gives the logits (search), the
hypothesis backtrack over the back-pointer tables (backtrack), and the helpers the tests share (the state block's layout, the inputs of the select
tests, the smallest decision gap of a step)."""
import numpy as np

DEAD = -1e9
ES = {False: 0, True: 1, 'never': 2}
# the select kernel's score against this restatement: fp32 log-sum over <= 2^15 terms in a tree with 2-ulp expf ~ 2e-6 absolute; l - max, - log sum
# and s + logp round once more each, 6e-8 relative
ABS_BAR, REL_BAR = 4e-6, 2.4e-7

# the device block in 4-byte words (gptq_mi355x.h)
W_EOS, W_MAX_NEW, W_LP, W_ES, W_T_CAP, W_BEAMS, W_T, W_OPEN, W_DONE, W_STATUS = range(10)
W_SCORE, W_PARENT, W_TOKEN, W_POOL, W_CAND, W_REC, W_TABLES = 16, 32, 48, 80, 160, 288, 1376


def f32(x):
    return np.asarray(x, dtype=np.float64).astype(np.float32).astype(np.float64)


class State:
    def __init__(self, n, max_new, eos=None, length_penalty=1.0, early_stopping=False, t_cap=None):
        self.n, self.max_new, self.eos = int(n), int(max_new), -1 if eos is None else int(eos)
        self.lp, self.es = float(np.float32(length_penalty)), ES[early_stopping]
        self.t_cap = self.max_new if t_cap is None else int(t_cap)
        self.t, self.open, self.done = 0, True, False
        self.score = np.array([0.0] + [DEAD] * (n - 1))
        self.parent = np.zeros(n, dtype=np.int64)
        self.token = np.zeros(n, dtype=np.int64)
        self.pool = [dict(score=DEAD, finished=False, step=0, parent=0, token=0) for _ in range(n)]
        self.cand = []                                   # the last step's 2N candidates (score, parent, token, hit)
        self.parent_at = np.zeros((self.t_cap, n), dtype=np.int64)
        self.token_at = np.zeros((self.t_cap, n), dtype=np.int64)

    def copy(self):
        import copy
        return copy.deepcopy(self)


def log_softmax(row):
    row = np.asarray(row, dtype=np.float64)
    m = row.max()
    return (row - m) - np.log(np.exp(row - m).sum())


def candidates(logits, score):
    """every (c, b, v) of the step in the rule's order: score descending, beam ascending, token ascending"""
    logits = np.asarray(logits, dtype=np.float64)
    n, vocab = logits.shape
    c = np.stack([f32(score[b] + log_softmax(logits[b])) for b in range(n)])
    order = np.lexsort((np.tile(np.arange(vocab), n), np.repeat(np.arange(n), vocab), -c.reshape(-1)))
    return c.reshape(-1), order


def min_gap(logits, score, n):
    """the smallest distinct gap among the best 2N + 1 candidate scores of the step (inf where all are equal)"""
    c, order = candidates(logits, score)
    top = c[order[:2 * n + 1]]
    d = -np.diff(top)
    d = d[d > 0]
    return float(d.min()) if d.size else float('inf')


def step(st, logits):
    """steps 1 .. 6 of the rule on N rows of logits, in place on `st`"""
    if st.done:
        return st
    n, t = st.n, st.t
    logits = np.asarray(logits, dtype=np.float64)
    vocab = logits.shape[1]
    assert logits.shape[0] == n and vocab >= 2 * n
    c, order = candidates(logits, st.score)
    top = order[:2 * n]
    cs, cb, cv = c[top], top // vocab, top % vocab
    hit = (cv == st.eos) | (t + 1 >= min(st.max_new, st.t_cap))
    m = np.where(hit, DEAD, cs)
    nxt = sorted(range(2 * n), key=lambda r: (-m[r], r))[:n]
    full = all(e['finished'] for e in st.pool)
    merged = [(e['score'], 0, i, e) for i, e in enumerate(st.pool)]
    for r in range(n):
        if hit[r] and st.open and not (full and st.es == 1):
            s = float(f32(cs[r] / float(t + 1) ** st.lp))
            merged.append((s, 1, r, dict(score=s, finished=True, step=t, parent=int(cb[r]), token=int(cv[r]))))
    merged.sort(key=lambda x: (-x[0], x[1], x[2]))
    st.pool = [x[3] for x in merged[:n]]
    st.score = np.array([m[r] for r in nxt])
    st.parent = np.array([cb[r] for r in nxt], dtype=np.int64)
    st.token = np.array([cv[r] for r in nxt], dtype=np.int64)
    st.parent_at[t], st.token_at[t] = st.parent, st.token
    st.cand = [(float(cs[r]), int(cb[r]), int(cv[r]), bool(hit[r])) for r in range(2 * n)]
    st.t = t + 1
    L = st.max_new if (st.es == 2 and st.lp > 0) else st.t
    best = st.score[0] / float(L) ** st.lp
    worst = min(e['score'] for e in st.pool)
    st.open = bool(st.open and any(best > (worst if e['finished'] else DEAD) for e in st.pool))
    full = all(e['finished'] for e in st.pool)
    st.done = not (st.open and not (full and st.es == 1) and not bool(hit.all()))
    return st


def backtrack(entry, parent_at, token_at):
    """the tokens of a pool entry, its closing token included"""
    toks = [0] * (entry['step'] + 1)
    toks[-1], beam = int(entry['token']), int(entry['parent'])
    for u in range(entry['step'] - 1, -1, -1):
        toks[u], beam = int(token_at[u][beam]), int(parent_at[u][beam])
    return toks


def result(st):
    """[(tokens, score)] of the finished pool entries, best first"""
    return [(backtrack(e, st.parent_at, st.token_at), e['score']) for e in st.pool if e['finished']]


def beams_tokens(st):
    """the N running beams' token lists so far"""
    out = []
    for b in range(st.n):
        toks, beam = [], b
        for u in range(st.t - 1, -1, -1):
            toks.append(int(st.token_at[u][beam]))
            beam = int(st.parent_at[u][beam])
        out.append(toks[::-1])
    return out


def search(logits_fn, n, max_new, eos=None, length_penalty=1.0, early_stopping=False):
    """the whole search: logits_fn(list of N token lists generated so far) -> [N, vocab] logits.  Returns the final State."""
    st = State(n, max_new, eos, length_penalty, early_stopping)
    while not st.done:
        step(st, logits_fn(beams_tokens(st)))
    return st


# ---- the device block ----
def state_words(n, t_cap):
    return W_TABLES + 2 * t_cap * n


def pack(st):
    """the State as the int32 words of the device block"""
    w = np.zeros(state_words(st.n, st.t_cap), dtype=np.int32)
    f = w.view(np.float32)
    w[W_EOS], w[W_MAX_NEW], f[W_LP], w[W_ES], w[W_T_CAP], w[W_BEAMS] = st.eos, st.max_new, st.lp, st.es, st.t_cap, st.n
    w[W_T], w[W_OPEN], w[W_DONE] = st.t, int(st.open), int(st.done)
    f[W_SCORE:W_SCORE + 16] = DEAD
    f[W_SCORE:W_SCORE + st.n] = st.score
    w[W_PARENT:W_PARENT + st.n] = st.parent
    w[W_TOKEN:W_TOKEN + 32].view(np.int64)[:st.n] = st.token
    for i in range(16):
        e = st.pool[i] if i < st.n else dict(score=DEAD, finished=False, step=0, parent=0, token=0)
        o = W_POOL + 5 * i
        f[o] = e['score']
        w[o + 1:o + 5] = int(e['finished']), e['step'], e['parent'], e['token']
    w[W_TABLES:W_TABLES + st.t_cap * st.n] = st.parent_at.reshape(-1)
    w[W_TABLES + st.t_cap * st.n:] = st.token_at.reshape(-1)
    return w


def unpack(w):
    """what the tests compare of a downloaded block, as a dict"""
    w = np.asarray(w, dtype=np.int32)
    f = w.view(np.float32)
    n, t_cap = int(w[W_BEAMS]), int(w[W_T_CAP])
    pool = []
    for i in range(n):
        o = W_POOL + 5 * i
        pool.append(dict(score=float(f[o]), finished=bool(w[o + 1]), step=int(w[o + 2]), parent=int(w[o + 3]), token=int(w[o + 4])))
    cand = [(float(f[W_CAND + 4 * r]), int(w[W_CAND + 4 * r + 1]), int(w[W_CAND + 4 * r + 2]), bool(w[W_CAND + 4 * r + 3])) for r in range(2 * n)]
    return dict(n=n, t_cap=t_cap, t=int(w[W_T]), open=bool(w[W_OPEN]), done=bool(w[W_DONE]), status=int(w[W_STATUS]),
                score=f[W_SCORE:W_SCORE + n].astype(np.float64), parent=w[W_PARENT:W_PARENT + n].astype(np.int64),
                token=w[W_TOKEN:W_TOKEN + 32].view(np.int64)[:n].copy(), pool=pool, cand=cand,
                parent_at=w[W_TABLES:W_TABLES + t_cap * n].reshape(t_cap, n).astype(np.int64),
                token_at=w[W_TABLES + t_cap * n:W_TABLES + 2 * t_cap * n].reshape(t_cap, n).astype(np.int64))


def from_words(w):
    """the State a downloaded block holds"""
    u = unpack(w)
    w = np.asarray(w, dtype=np.int32)
    st = State(u['n'], int(w[W_MAX_NEW]), None if w[W_EOS] < 0 else int(w[W_EOS]), float(w.view(np.float32)[W_LP]),
               {0: False, 1: True, 2: 'never'}[int(w[W_ES])], u['t_cap'])
    st.t, st.open, st.done, st.score, st.parent, st.token = u['t'], u['open'], u['done'], u['score'], u['parent'], u['token']
    st.pool, st.parent_at, st.token_at = u['pool'], u['parent_at'], u['token_at']
    return st


def close(a, b):
    return a == b or abs(a - b) <= ABS_BAR + REL_BAR * abs(b)             # (a == b: -inf against -inf)


def same_step(got, st, scores=True):
    """the downloaded block `got` (unpack) against the oracle State behind the same step: exact parents, tokens, flags and pool entries, scores
    within the bar.  Returns a message, or None where they agree."""
    if (got['t'], got['open'], got['done']) != (st.t, st.open, st.done):
        return 'flags %r != %r' % ((got['t'], got['open'], got['done']), (st.t, st.open, st.done))
    if got['parent'].tolist() != st.parent.tolist() or got['token'].tolist() != st.token.tolist():
        return 'beams %r %r != %r %r' % (got['parent'].tolist(), got['token'].tolist(), st.parent.tolist(), st.token.tolist())
    if [c[1:] for c in got['cand']] != [c[1:] for c in st.cand]:
        return 'candidates %r != %r' % (got['cand'], st.cand)
    for a, b in zip(got['pool'], st.pool):
        if (a['finished'], a['step'], a['parent'], a['token']) != (b['finished'], b['step'], b['parent'], b['token']):
            return 'pool %r != %r' % (got['pool'], st.pool)
    if scores:
        pairs = list(zip(got['score'], st.score)) + [(a['score'], b['score']) for a, b in zip(got['pool'], st.pool)] + \
            [(a[0], b[0]) for a, b in zip(got['cand'], st.cand)]
        for a, b in pairs:
            if not close(a, b):
                return 'score %r != %r' % (a, b)
    return None


# ---- the inputs of the select tests ----
SELECT_SHAPES = ((2, 8), (3, 1003), (4, 1000), (8, 512), (5, 32001), (16, 32000))


def select_inputs(n, vocab, seed=0):
    rng = np.random.default_rng(1000 * n + seed)
    logits = (rng.standard_normal((n, vocab)) * 3).astype(np.float16)
    score = np.sort(-rng.uniform(0, 2, n))[::-1].astype(np.float32)
    return logits, score
