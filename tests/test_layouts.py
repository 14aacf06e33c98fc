"""CPU: the LDS layouts the kernels rely on are conflict-free under the gfx950 ds_read_b128 lane-group model
(MI355X_MICROARCH.md section LDS: 4 groups of 16 lanes, bank = (addr/4) % 64)."""
from collections import defaultdict

G0 = list(range(0, 4)) + list(range(12, 16)) + list(range(20, 28))
G1 = list(range(4, 12)) + list(range(16, 20)) + list(range(28, 32))
GROUPS = [G0, G1, [32 + x for x in G0], [32 + x for x in G1]]


def b128_cycles(addr_of_lane):
    tot = 0
    for g in GROUPS:
        banks = defaultdict(set)
        for l in g:
            a = addr_of_lane(l)
            assert a % 16 == 0
            for b in range(4):
                banks[(a // 4 + b) % 64].add(a)
        tot += max(len(s) for s in banks.values())
    return tot


def test_igemm_fragment_reads_are_conflict_free():
    # csrc/igemm.hip compute(): lane reads row (lane&31), 16-byte slot (2q + lane>>5) ^ ((row>>1)&7), 128-byte rows
    for q in range(4):
        assert b128_cycles(lambda l: (l & 31) * 128 + (((2 * q + (l >> 5)) ^ (((l & 31) >> 1) & 7)) * 16)) == 4
    # and the un-swizzled layout would be an 8-way conflict (why the swizzle exists)
    assert b128_cycles(lambda l: (l & 31) * 128 + (l >> 5) * 16) == 32


def test_igemm_swizzle_is_a_bijection_per_row():
    for row in range(256):
        assert sorted(s ^ ((row >> 1) & 7) for s in range(8)) == list(range(8))


def test_bilstm_h_reads_are_conflict_free():
    # csrc/bilstm.hip: lane reads h[row = lane&15][16qq + 4*(lane>>4) .. +3], row pitch 136 floats
    for qq in range(8):
        assert b128_cycles(lambda l: (l & 15) * 544 + 64 * qq + 16 * (l >> 4)) == 4
    assert b128_cycles(lambda l: (l & 15) * 512 + 16 * (l >> 4)) > 4


def test_xcd_block_remap_is_bijective():
    # csrc/igemm.hip: lid = (xcd < r ? xcd*(q+1) : r*(q+1) + (xcd-r)*q) + bid/8
    for nblk in list(range(1, 70)) + [518 * 4, 2072, 33750 * 2 + 3]:
        q, r = nblk >> 3, nblk & 7
        seen = set()
        for bid in range(nblk):
            xcd = bid & 7
            lid = (xcd * (q + 1) if xcd < r else r * (q + 1) + (xcd - r) * q) + (bid >> 3)
            assert 0 <= lid < nblk
            seen.add(lid)
        assert len(seen) == nblk


def _tw16_col(l31):
    return ((l31 - 2) & 15) if (l31 & 16) else l31      # csrc/conv3x3.hip c3_tw16_col


def test_conv3x3_window_reads_conflict_free_for_both_patch_shapes():
    """csrc/conv3x3.hip compute(): lane reads LDS row r = tilebase + ky*PW + kx, slot (2q + lane>>5) ^ ((r>>1)&7). A lane
    group is conflict-free iff its 16 rows are distinct mod 16: true for 32 consecutive rows (8 x 32 patches, flat windows)
    and, for 16 x 16 patches (pitch 18), only with the second row's lanes rotated by two columns."""
    def cycles(row_of_l31, q):
        def addr(l):
            r = row_of_l31(l & 31)
            return r * 128 + (((2 * q + (l >> 5)) ^ ((r >> 1) & 7)) * 16)
        return b128_cycles(addr)

    for q in range(4):
        for tap_off in (0, 1, 2, 34, 35, 36, 70):                       # ky * 34 + kx of the 8 x 32 patch
            for tile in range(8):
                assert cycles(lambda l: tile * 34 + l + tap_off, q) == 4
        for tap_off in (0, 1, 2, 18, 19, 20, 36, 37, 38):                # ky * 18 + kx of the 16 x 16 patch
            for tile in range(8):
                rot = lambda l: (2 * tile + (l >> 4)) * 18 + _tw16_col(l) + tap_off
                plain = lambda l: (2 * tile + (l >> 4)) * 18 + (l & 15) + tap_off
                assert cycles(rot, q) == 4
                assert cycles(plain, q) > 4                                  # what SQ_LDS_BANK_CONFLICT saw before the rotation
    # the rotation is a permutation of the 16 columns of the second row, identity on the first
    assert sorted(_tw16_col(l) for l in range(16, 32)) == list(range(16)) and [_tw16_col(l) for l in range(16)] == list(range(16))


def _b32_cycles(addr_of_lane):
    """ds_read_b32 / ds_read2_b32 halves: two groups of 32 lanes, bank = (addr/4) % 32."""
    tot = 0
    for g in (range(0, 32), range(32, 64)):
        banks = defaultdict(set)
        for l in g:
            a = addr_of_lane(l)
            banks[(a // 4) % 32].add(a // 4)
        tot += max(len(s) for s in banks.values())
    return tot


def test_conv_first_plane_copies_sit_on_complementary_banks():
    """csrc/conv_first.hip conv_first_mfma_kernel: lane l31 reads 4 dwords at element 3 * l31 (+ 8 for lanes 32..63) of a bf16 plane,
    even lanes from copy A, odd lanes from copy B (one element later, CF_PLANE elements further): with (CF_PLANE / 2) % 32 == 14
    the odd lanes' dwords fall on the 16 banks the even lanes leave free."""
    CF_ROW_B, CF_NEL = 198, 6 * 198
    for plane in (CF_NEL + 56, CF_NEL + 20):
        worst = 0
        for wave in range(4):
            for dword in range(4):
                def addr(l):
                    l31, fh = l & 31, l >> 5
                    par = l31 & 1
                    s0 = wave * CF_ROW_B + 3 * l31 + 8 * fh
                    return 4 * (((par * plane + s0 + par) >> 1) + dword)
                worst = max(worst, _b32_cycles(addr))
        if plane == CF_NEL + 56:
            assert (plane // 2) % 32 == 14 and worst == 2        # one LDS cycle per 32-lane half
        else:
            assert worst > 2                                      # the first layout (plane = 1208) was 2-way conflicted


def test_bilstm_split_h_planes_conflict_free():
    # csrc/bilstm.hip bilstm_split_kernel: lane reads 8 bf16 (16 B) at h[row = lane&15][32 kk + 8 (lane>>4)], row pitch 288 B
    for kk in range(4):
        assert b128_cycles(lambda l: (l & 15) * 288 + 64 * kk + 16 * (l >> 4)) == 4
    assert b128_cycles(lambda l: (l & 15) * 272 + 16 * (l >> 4)) > 4       # the "natural" 256 + 16 pitch is not


def test_fused_conv1_producer_covers_the_window_and_stays_inside_its_buffers():
    """csrc/conv3x3_wr.h, conv3x3_wr_kernel<FUSE>: the index arithmetic of the conv1_1 producer, restated. A tile's 10 x 34-pixel window
    is produced by 4 waves x 3 groups of 32 lanes; every window pixel must be written (some twice, with the same value), every write must
    land inside the 48-KiB window buffer at the 144-byte pitch, every operand read inside the 12 x 36-pixel q patch (the plane), and the
    patch's 216 sixteen-byte chunks must be fetched exactly once by the one LDS-DMA per wave."""
    WR_PW, WR_PITCH, WR_WIN = 34, 144, 48 * 1024
    FQ_PW, FQ_ROWB, FQ_PLANE = 36, 36 * 8, 4096
    goff = (0, 32, 53)
    written = set()
    for wave in range(4):
        for gi in range(3):
            for lane in range(64):
                l31, fhalf = lane & 31, lane >> 5
                p = 85 * wave + goff[gi] + l31
                assert 0 <= p < 10 * WR_PW
                r, c = divmod(p, WR_PW)
                # operands: two consecutive q pixels starting at patch column c + fhalf of patch rows r + ky
                for ky in range(3):
                    a = ((r + ky) * FQ_PW + c + fhalf) * 8
                    assert a % 8 == 0 and a + 16 <= 12 * FQ_ROWB <= FQ_PLANE
                    assert (a // FQ_ROWB) == r + ky and (a + 15) // FQ_ROWB == r + ky       # both pixels in the same patch row
                # results: channels 32 i + 8 h + 4 fhalf .. + 3 (8 bytes) of window pixel p
                base = (85 * wave + l31) * WR_PITCH + 8 * fhalf
                for i in range(2):
                    for h in range(4):
                        w = base + goff[gi] * WR_PITCH + 64 * i + 16 * h
                        assert w == p * WR_PITCH + (32 * i + 8 * h + 4 * fhalf) * 2 and w + 8 <= WR_WIN
                        written.update(range(w, w + 8))
    for p in range(10 * WR_PW):                                   # all 128 data bytes of every window pixel; the 16 pad bytes stay untouched
        assert all(p * WR_PITCH + b in written for b in range(128)) and not any(p * WR_PITCH + b in written for b in range(128, 144))
    # the patch DMA: chunk j = wave * 64 + lane (j >= 216 re-reads chunk 0), LDS byte 16 j of the plane, source row j // 18, bytes 16 (j % 18)
    got = [0] * 216
    for j in range(256):
        jj = j if j < 12 * (FQ_ROWB // 16) else 0
        row, cc = divmod(jj, FQ_ROWB // 16)
        assert row < 12 and cc * 16 + 16 <= FQ_ROWB
        if j < 216:
            assert 16 * j == row * FQ_ROWB + 16 * cc                # the plane is the patch, row-major at 288 bytes per row
            got[jj] += 1
    assert got == [1] * 216
