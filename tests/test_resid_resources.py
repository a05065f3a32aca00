"""Resource guard for the residual modes of the shared tile kernel (no GPU
needed): compiles ame_predict.hip at the widest latent dim for gfx950 and reads
the compiler's resource report.

MODE 6 (ame_resid_nodes) is the one with a register problem: MODE 0 already
holds 160 VGPRs, and nine fp64 sums for four row nodes and four column nodes do
not fit beside the 20 accumulators under __launch_bounds__(AME_NT, 2).  It adds
its sums a few slots per pass (3, 2 and 4) and must spill nothing.  Its column
partials (4 waves x 64 columns x 4 slots, 8 KB) and MODE 7's uint32 [2048]
histogram (8 KB) live inside their own branches, so modes 0 - 5 keep the LDS and
the registers they had before these modes existed.
"""
import pytest

from test_probit_resources import HIPCC, _check, _report

KERNEL = "ame_predict_pairs_kernelILi32ELi%dEE"
# (VGPRs, LDS bytes) of modes 0 - 5 at r = 32 before modes 6 - 8 were added
BEFORE = {0: (160, 18080), 1: (129, 17408), 2: (131, 18080), 3: (114, 18080), 4: (113, 33792), 5: (119, 17424)}


@pytest.fixture(scope="module")
def report(tmp_path_factory):
    if HIPCC is None:
        pytest.skip("hipcc not available")
    return _report("ame_predict.hip", tmp_path_factory.mktemp("resid") / "pr.o", ("-DAME_ONLY_R=32",))


@pytest.mark.parametrize("mode", (6, 7, 8), ids=("nodes", "hist", "select"))
def test_residual_modes_spill_nothing_and_keep_the_occupancy(report, mode):
    rep, = _check(report, KERNEL % mode, scratch=32)   # the body's four staging pointers, as in every mode
    print(f"MODE {mode}: {rep}")
    assert rep.get("VGPRs Spill") == 0 and rep.get("SGPRs Spill", 0) == 0, rep
    assert rep.get("LDS Size", 0) <= 65536, rep
    assert rep.get("Occupancy", 0) >= 2, rep
    assert rep.get("VGPRs", 0) + rep.get("AGPRs", 0) <= 256, rep


def test_new_lds_is_in_the_new_modes_only(report):
    lds = {m: _check(report, KERNEL % m, scratch=32)[0].get("LDS Size", 0) for m in range(9)}
    print(lds)
    assert lds[6] <= BEFORE[1][1] + 4 * 64 * 4 * 8      # operand tiles + the column partials
    assert lds[7] <= BEFORE[1][1] + 2048 * 4            # operand tiles + the histogram
    assert lds[8] <= BEFORE[5][1]


@pytest.mark.parametrize("mode", sorted(BEFORE))
def test_earlier_modes_keep_their_resources(report, mode):
    rep, = _check(report, KERNEL % mode, scratch=32)
    assert (rep.get("VGPRs"), rep.get("LDS Size")) == BEFORE[mode], (mode, rep)
