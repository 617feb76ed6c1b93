"""CPU test of the case table of tests/test_wino_tail_gpu.py: what its comments say about every length - the live pairs of the row's last
Winograd tile, on which side of the column-wave boundary they end - and that every launch has more than the 128 workgroups below which
v2w_conv1d_wino declines it.  No GPU needed."""
from tests import test_wino_tail_gpu as T


def test_case_table():
    for L, d, live in T.TAIL_CASES:
        assert T.tail_live_pairs(L, d) == live, (L, d, T.tail_live_pairs(L, d))
        assert T.workgroups(L, d) > 128, (L, d, T.workgroups(L, d))
    lives = {live for _L, d, live in T.TAIL_CASES if d == 3}
    assert {0, 32, 33} <= lives and any(0 < v < 32 for v in lives)      # full tiles, the dead second wave at its boundary, one live column


def test_a_dead_wave_has_no_live_column():
    """wino_tpos grows with the pair index, so a wave whose FIRST column starts at or past the end owns no output position below it."""
    for d in (1, 3, 5):
        t = [T.tpos(P, d) for P in range(2000)]
        assert all(a < b for a, b in zip(t, t[1:]))


def test_len_ends_sit_where_the_comments_say():
    d, P0 = 3, 5 * T.NTP
    assert (T.tpos(P0, d), T.tpos(P0 + 31, d), T.tpos(P0 + 32, d), T.tpos(P0 + 33, d)) == (638, 702, 703, 704)
    assert T.LEN_ENDS[:6] == [660, 703, 704, 720, 638, 639] and len(T.LEN_ENDS) == T.B
