"""The inputs of tests/test_gpu_spec_sample_batch.py, whose margins tests/test_host_spec_sample_batch.py checks on the CPU: every sequence of a batch
is a WINDOW of the 16-row case of spec_sample_ref.gpu_case -- rows o .. o + R - 1 of P, ids, T, k, p, ua, ud and rows o .. o + R - 2 of Q.  A row's
decision depends on its own target row, draft row, draft and uniforms only, so the margins of the 16-row case carry over; a window's last row
becomes a bonus row, which uses its top-p margin alone.  Nothing here imports the product."""
import spec_sample_ref as X

FULL = 16
VOCABS, ROWS = (50, 257, 32001), (2, 5, 8)


def window(V, R, with_q, o):
    """rows o .. o + R - 1 of the 16-row case as a case of R rows: dict(P, Q, ids, T, k, p, ua, ud)"""
    assert 0 <= o <= FULL - R
    c = X.gpu_case(V, FULL, with_q)
    w = {n: c[n][o:o + R] for n in ('P', 'ids', 'T', 'k', 'p', 'ua', 'ud')}
    w['Q'] = c['Q'][o:o + R - 1] if with_q else None
    return w


def offsets(R, B):
    """the windows of a batch of B: first, middle and last for B = 3 (distinct), all 17 - R in turn for more sequences than there are windows"""
    n = FULL - R + 1
    return [0, (FULL - R) // 2, FULL - R] if B == 3 else [b % n for b in range(B)]


def batch(V, R, with_q, B):
    return [window(V, R, with_q, o) for o in offsets(R, B)]


def oracle(w):
    """(a, emitted, flags, tokens) of a window by the float64 oracle"""
    return X.verify(w['P'], w['ids'], w['Q'], w['T'], w['k'], w['p'], w['ua'], w['ud'])


def admissible(w, flags, tokens):
    return X.admissible(flags, tokens, w['P'], w['ids'], w['Q'], w['T'], w['k'], w['p'], w['ua'], w['ud'])
