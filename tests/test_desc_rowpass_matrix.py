"""The constant operand of k_desc's matrix-core row pass, as the host builds it (orbx_desc_rowpass_matrix), in numpy, without a GPU:
the B fragments times a biased random patch, laid out and read exactly as the kernel reads its LDS, plus the accumulator constant,
are the exact row sums of the 7-tap filter -- and, run through the column pass, the blur of front_model.blur7_model -- for both tap
profiles."""
import numpy as np
import pytest

import front_model as fm

RP = 48     # raw pitch of the kernel's LDS patch in its matrix-core form


def _row_pass_as_the_kernel(lds, B, acc0):
    """lds: the flat LDS bytes.  A fragment of row tile mt: lane l reads 16 bytes at (16 mt + l % 16) * RP + 16 (l / 16), XOR 0x80, signed.
    The instruction multiplies byte j of lane (row + 16 q) of A with byte j of lane (column + 16 q) of B, q = 0..3, and sums."""
    out = np.zeros((48, 48), np.int64)
    Bs = B.astype(np.int8).astype(np.int64)                                  # [tile, lane, j]
    for mt in range(3):
        A = np.zeros((64, 16), np.int64)
        for l in range(64):
            at = (16 * mt + l % 16) * RP + 16 * (l // 16)
            A[l] = (lds[at:at + 16] ^ 0x80).astype(np.int8)
        A4 = A.reshape(4, 16, 16)                                            # [q, row, j]
        for nt in range(3):
            B4 = Bs[nt].reshape(4, 16, 16)                                   # [q, column, j]
            out[16 * mt:16 * mt + 16, 16 * nt:16 * nt + 16] = np.einsum("qrj,qcj->rc", A4, B4) + acc0
    return out


@pytest.mark.parametrize("profile", [0, 1])
def test_rowpass_matrix_gives_the_exact_row_sums(pkg, profile):
    B, acc0 = pkg.orbx.desc_rowpass_matrix(profile)
    taps = fm.gaussian_taps(profile)
    assert B.shape == (3, 64, 16) and acc0 == 128 * int(taps.sum()) and acc0 == (32896, 32768)[profile]
    assert int(B.max()) == int(taps.max()) and B.max() < 128                 # signed bytes in the instruction
    # the banded matrix itself: G[k][c] = taps[k - c]
    G = np.zeros((64, 48), np.int64)
    for t in range(3):
        for l in range(64):
            G[16 * (l // 16):16 * (l // 16) + 16, 16 * t + l % 16] = B[t, l]
    want = np.zeros((64, 48), np.int64)
    for c in range(37):
        want[c:c + 7, c] = taps
    assert (G == want).all()
    rng = np.random.default_rng(17 + profile)
    for trial in range(3):
        # every LDS byte random, the never-staged ones (columns 43..47, rows 43..47 and beyond) included: they must not reach a result
        lds = rng.integers(0, 256, 48 * RP + 64, dtype=np.uint8)
        patch = lds[:43 * RP].reshape(43, RP)[:, :43].copy()
        if trial == 1:
            patch[:] = 255
        if trial == 2:
            patch[:] = 0
        lds[:43 * RP].reshape(43, RP)[:, :43] = patch
        R = _row_pass_as_the_kernel(lds, B, acc0)[:43, :37]
        rows = sum(int(taps[k]) * patch[:, k:k + 37].astype(np.int64) for k in range(7))
        assert (R == rows).all()
        assert R.min() >= 0 and R.max() <= 65535 and (trial != 1 or R.max() == 255 * int(taps.sum()))
        # through the column pass: the interior of the blurred patch
        full = sum(int(taps[k]) * R[k:k + 37, :] for k in range(7))
        blurred = np.minimum((full + (1 << 15)) >> 16, 255).astype(np.uint8)
        assert (blurred == fm.blur7_model(patch, profile)[3:40, 3:40]).all()
