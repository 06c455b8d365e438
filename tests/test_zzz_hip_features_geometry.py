"""features.logmelfilterbank / loudness_extract on the MI355X, dense and ragged, at the geometries that give the STFT
plan (features._Stft) the shapes the recipe's geometry of tests/test_hip_features_ragged.py does not: signal rows every
4, 8 and 16 samples, the generic contraction kernel, one to 32 tap groups chained through RES_ADD, the function's own
defaults, more mels than srn_logmel's workgroup and than bins, an odd n_fft - win_length.  Cases, reference
(oracle/features_oracle.py on the unpadded item) and the derived bounds are tests/_features_ragged_cases.py's; the CPU
suite runs the same list through the C-ABI emulator (tests/test_features_ragged_emulated.py) and asserts the plan shape
each geometry produces.

The file's name sorts it behind the test files that were there before it."""
import pytest

from tests import _features_ragged_cases as C

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.mark.parametrize("geom", list(C.GEOMETRIES), ids=lambda g: "fft{}-hop{}-win{}-mels{}".format(*g))
def test_geometry_logmel_meets_the_oracle(geom):
    C.check_geometry("mel", geom, C.geometry_mel_errors(geom, DEV))


@pytest.mark.parametrize("mode", C.PAD_MODES)
@pytest.mark.parametrize("hop", list(C.LOUD_HOPS))
def test_geometry_loudness_meets_the_oracle(hop, mode):
    C.check_geometry("loud", (hop, mode), C.geometry_loud_errors(hop, mode, DEV))
