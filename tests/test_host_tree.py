"""CPU-side tests of tree speculative decoding: prompt_lookup_tree_draft and the validation of DecodeEngine.set_tree (quant/decode.py)."""
import pytest

from quant.decode import DecodeEngine, prompt_lookup_draft, prompt_lookup_tree_draft


def test_one_occurrence_is_the_chain():
    seq = [7, 1, 2, 5, 6, 9, 1, 2]
    toks, parents = prompt_lookup_tree_draft(seq, 5, max_ngram=3, width=3)
    assert toks == prompt_lookup_draft(seq, 4, max_ngram=3) and parents == [0, 1, 2, 3]
    assert prompt_lookup_tree_draft([1, 2, 3], 4) == ([3, 3, 3], [0, 1, 2])            # no occurrence: the chain's repeats


def test_two_occurrences_share_their_common_first_token():
    # [1, 2] was followed by 3, 4, 8, 0, 1, 2 and, earlier, by the longer 3, 5, 9, ..: node 1 (token 3) is shared, the longer run goes first below it
    seq = [1, 2, 3, 5, 9, 0, 1, 2, 3, 4, 8, 0, 1, 2]
    toks, parents = prompt_lookup_tree_draft(seq, 16, max_ngram=2, width=3)
    assert toks[:3] == [3, 5, 4] and parents[:3] == [0, 1, 1]
    assert all(0 <= q <= i for i, q in enumerate(parents))                                # topological: a parent is the root or an earlier draft
    assert len({(q, t) for q, t in zip(parents, toks)}) == len(toks)                      # a trie: no two children of a node carry one token


def test_the_node_budget_is_respected():
    seq = [1, 2, 3, 5, 9, 0, 1, 2, 3, 4, 8, 0, 1, 2, 6, 6, 6, 0, 1, 2]
    for nodes in (1, 2, 3, 4, 6, 16):
        toks, parents = prompt_lookup_tree_draft(seq, nodes, max_ngram=2, width=3)
        assert len(toks) == len(parents) <= nodes - 1
        assert nodes < 4 or (sorted(toks[:2]) == [3, 6] and parents[:2] == [0, 0])          # level by level: every branch before any second token


def test_set_tree_refuses_a_parent_array_that_is_not_topological():
    eng = object.__new__(DecodeEngine)                      # the validation runs ahead of every upload: no device is needed
    eng.chunk, eng.batch_chunk, eng.tree = 5, 0, True
    for parents in ([-1, 2, 0], [0, 0, 1], [-1, 0, 2], [-1, 0]):
        with pytest.raises(ValueError):
            eng.set_tree([4, 5, 6], parents)
    with pytest.raises(ValueError):
        eng.set_tree([1] * 6, [-1, 0, 1, 2, 3, 4])          # more nodes than chunk rows
