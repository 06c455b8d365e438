"""One whole-model training step issues the launches recorded in tests/golden/train_step_trace.json: the same entry
points, in the same order, with the same arguments on the same buffers (tests/golden/make_golden_train_trace.py states
the step and the signature).  The fixture is a constant: a change to the training path that is meant to leave the
launches alone must reproduce it byte for byte."""
import collections
import json

from tests.golden import make_golden_train_trace as G


def test_training_step_issues_the_recorded_launches():
    with open(G.FIXTURE) as f:
        text = f.read()
    want = json.loads(text)
    count = collections.Counter(name for name, _ in want)
    assert len(want) == 529
    assert (count["srn_conv_gemm"], count["srn_tn_gemm"], count["srn_chunk_colsum"], count["srn_transpose_ct"]) == \
        (198, 101, 31, 25)
    assert (count["srn_multi_copy"], count["srn_transpose_multi"], count["srn_sumsq"], count["srn_adamw"]) == (1, 3, 1, 1)
    got = G.trace()
    sig = json.loads(json.dumps(got))
    for i, (a, b) in enumerate(zip(sig, want)):
        assert a == b, f"launch {i} differs: {a[0]} / recorded {b[0]}"
    assert len(sig) == len(want), f"launch {min(len(sig), len(want))} differs (one trace ends there)"
    assert G.dumps(got) == text
