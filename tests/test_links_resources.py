"""Resource guard for the link-ranking modes of the shared tile kernel (no GPU
needed): compiles ame_predict.hip at the widest latent dim for gfx950 and reads
the compiler's resource report.

MODE 4 (ame_probit_rank) adds a uint32 [2][2048] histogram (16 KB) to the tile
kernel's LDS, MODE 5 (ame_probit_select) two words.  Both keep
__launch_bounds__(AME_NT, 2): with the histogram a workgroup must stay within
the 64 KB it may declare statically and leave room for two workgroups per CU,
spill no VGPR and use no scratch beyond the 32 bytes every mode of this body
has (test_probit_resources.py).
"""
import pytest

from test_probit_resources import HIPCC, _check, _report

KERNEL = "ame_predict_pairs_kernelILi32ELi%dEE"


@pytest.fixture(scope="module")
def report(tmp_path_factory):
    if HIPCC is None:
        pytest.skip("hipcc not available")
    return _report("ame_predict.hip", tmp_path_factory.mktemp("links") / "pr.o", ("-DAME_ONLY_R=32",))


@pytest.mark.parametrize("mode", (4, 5), ids=("rank", "select"))
def test_link_modes_spill_nothing_and_keep_the_occupancy(report, mode):
    base, = _check(report, KERNEL % 0, scratch=32)          # <32, 0>: Gaussian scoring
    rep, = _check(report, KERNEL % mode, scratch=min(32, base.get("ScratchSize", 0)))
    print(f"MODE {mode}: {rep}; MODE 0: {base}")
    assert rep.get("LDS Size", 0) <= 65536, rep
    assert rep.get("Occupancy", 0) >= base.get("Occupancy", 0), (rep, base)
    assert rep.get("Occupancy", 0) >= 2, rep


def test_the_histogram_is_in_the_rank_mode_only(report):
    """Modes 0 - 3 and 5 do not pay for MODE 4's 16 KB of LDS."""
    lds = {m: _check(report, KERNEL % m, scratch=32)[0].get("LDS Size", 0) for m in (0, 3, 4, 5)}
    print(lds)
    assert lds[4] >= 2 * 2048 * 4 and lds[4] - 2 * 2048 * 4 <= lds[0]
    assert lds[3] <= lds[0] and lds[5] <= lds[0]
