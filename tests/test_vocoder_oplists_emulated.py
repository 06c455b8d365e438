"""Every HiFi-GAN / SiFiGAN plan emits the op list recorded in tests/golden/vocoder_oplists.json: the same entry points,
in the same order, with the same arguments on the same buffers (tests/golden/make_golden_oplists.py states the
signature).  The fixture is a constant: a change to the plan builders that is meant to leave the plans alone must
reproduce it byte for byte."""
import json

from tests.golden import make_golden_oplists as G


def test_every_plan_emits_the_recorded_op_list():
    with open(G.FIXTURE) as f:
        text = f.read()
    want = json.loads(text)
    got = G.signatures()
    assert list(got) == list(want)
    assert [len(want[n]) for n in list(want)[:2] + list(want)[4:8]] == [23, 23, 74, 74, 36, 36]
    for name, sig in got.items():
        sig = json.loads(json.dumps(sig))
        for i, (a, b) in enumerate(zip(sig, want[name])):
            assert a == b, f"{name}: op {i} differs"
        assert len(sig) == len(want[name]), f"{name}: op {min(len(sig), len(want[name]))} differs (one list ends there)"
    assert G.dumps(got) == text
