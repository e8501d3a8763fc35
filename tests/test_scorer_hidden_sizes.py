"""CPU: which hidden sizes the fp32 edge scorer takes (sgs_edge_score_hidden_supported, a host-only predicate) and that the header
parser binds it."""
import pytest


@pytest.fixture(scope="module")
def L():
    import sgs_gnn_amd
    return sgs_gnn_amd._lib.lib()


def test_header_declares_the_predicate():
    import sgs_gnn_amd
    protos = sgs_gnn_amd._lib.parse_header()
    assert "sgs_edge_score_hidden_supported" in protos
    _, argtypes, argnames = protos["sgs_edge_score_hidden_supported"]
    assert len(argtypes) == 1 and argnames == ["H"]


@pytest.mark.parametrize("H,ok", [(0, 0), (2, 0), (4, 1), (6, 0), (64, 1), (100, 1), (256, 1), (260, 0), (288, 1), (300, 0), (320, 1),
                                  (352, 1), (384, 1), (512, 1), (514, 0), (640, 1), (1000, 0), (1024, 1), (1056, 0), (2048, 0), (-32, 0)])
def test_hidden_supported_table(L, H, ok):
    assert L.sgs_edge_score_hidden_supported(H) == ok


def test_paired_supported_covers_the_wide_sizes(L):
    assert [L.sgs_edge_score_paired_supported(H) for H in (64, 128, 256, 288, 300, 512, 1024, 1056)] == [0, 1, 1, 1, 0, 1, 1, 0]
    # the bf16 mode, the mask form and the dfeat row GEMM stay H = 128 / 256
    for H in (384, 512, 1024):
        assert not L.sgs_edge_score_bf16_supported(H)
        assert not L.sgs_edge_score_bwd_bits_supported(H)
        assert not L.sgs_edge_score_bwd_dfeat_supported(H)


def test_wide_sizes_pass_argument_validation(L):
    """With no edges the entry points validate and return: H = 512 passes, H = 300 and 1056 report 'unsupported'."""
    assert L.sgs_edge_score_fwd(None, None, 10, 512, None, 0, 0, None, None, None, None, 0.0, 0, 0, None, None, 0, None) == 0
    for H in (300, 1056):
        rc = L.sgs_edge_score_fwd(None, None, 10, H, None, 5, 0, None, None, None, None, 0.0, 0, 0, None, None, 0, None)
        assert rc == -1 and b"unsupported" in L.sgs_last_error()
