"""The model of the matrix-core nomination family (tests/batch_ref.py) and the certificate's margin (host/vt_batchbound.h),
on the CPU.

batch_group_finish certifies a query on the premise that every score a nomination kernel forms is within `eps` of the true
one.  test_gpu_batch_kernels.py holds the kernels to that, with tolerances from the library's own function; here

  * that function is built stand-alone (tests/batchbound_check.cpp, g++ with AddressSanitizer and UBSan), checks itself and
    prints its values on a grid, which must be the model's own derivation of the margin;
  * the model's bf16 rounding is torch's, its images are permutations that put the documented element in the documented slot;
  * on every input class the kernel tests use, a plain machine -- operands rounded to bf16, products added one by one in f32
    -- stays inside the margin's terms around the f64 truth: the classes are ones on which the bound can be met at all, so a
    kernel that misses it there is wrong, not unlucky.
"""
import os
import subprocess
import tempfile

import numpy as np
import pytest

import batch_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_margin_function_under_sanitizers_is_the_models_derivation():
    exe = os.path.join(tempfile.mkdtemp(), "batchbound_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off",
                           "-fsanitize=address,undefined", os.path.join(ROOT, "tests", "batchbound_check.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    lines = out.stdout.split("\n")
    assert out.returncode == 0 and lines[-2] == "ok", (out.stdout[-2000:], out.stderr[-2000:])
    rows = [ln.split() for ln in lines[:-2]]
    assert len(rows) == 2 * 8 * 8 * 8

    def same(a, b):  # the two are the same formula in two orders: a few units in the last place
        return a == b or abs(a - b) <= 1e-14 * abs(b)

    for f in rows:
        l2, d = int(f[0]), int(f[1])
        qn, xn, e32, e16, rnd, acc, fl = (float.fromhex(x) for x in f[2:])
        want = ref.bf16_terms(l2, d, qn, xn)
        assert same(rnd, want[0]) and same(acc, want[1]) and same(fl, want[2]), f
        assert same(e16, ref.eps(l2, True, d, qn, xn)) and same(e32, ref.eps(l2, False, d, qn, xn)), f


def test_bf16_rounding_is_nearest_even():
    one = np.float32(1.0)
    cases = [(one, 0x3F80), (one + np.float32(2.0 ** -8), 0x3F80),            # a tie: down to the even mantissa
             (one + np.float32(2.0 ** -8 + 2.0 ** -23), 0x3F81),              # just above the tie
             (one + np.float32(3 * 2.0 ** -8), 0x3F82),                       # a tie: up to the even mantissa
             (np.float32(-0.0), 0x8000), (np.float32(np.inf), 0x7F80), (np.float32(3.4e38), 0x7F80),  # rounds to inf
             (np.float32(1e-45), 0x0000), (np.float32(1e-40), 0x0001)]        # subnormals: the same rule on the bits
    for x, bits in cases:
        assert int(ref.bf16_bits(np.array([x]))[0]) == bits, (x, hex(bits))
    import torch
    rng = np.random.default_rng(5)
    x = np.concatenate([rng.standard_normal(20000).astype(np.float32), (rng.standard_normal(20000) * 1e-39).astype(np.float32),
                        (rng.standard_normal(20000) * 1e15).astype(np.float32), rng.integers(0, 0x7F800000, 20000).astype(np.uint32).view(np.float32)])
    got = ref.bf16_bits(x)
    want = torch.from_numpy(x).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
    assert np.array_equal(got, want)
    assert np.array_equal(ref.bf16_round(x).view(np.uint32), got.astype(np.uint32) << 16)


def distinct_matrix(rows, ld):
    """f32 values whose bf16 images are all different and finite (the bit patterns 0x0080 .. of bf16, in order)"""
    bits = (np.arange(rows * ld, dtype=np.uint32) + 0x0080) << 16
    assert rows * ld + 0x0080 < 0x7F80
    return bits.view(np.float32).reshape(rows, ld)


@pytest.mark.parametrize("ld,nq_pad", [(64, 64), (128, 256), (192, 128)])
def test_query_images_are_permutations_with_the_documented_slots(ld, nq_pad):
    if nq_pad * ld + 0x80 >= 0x7F80:
        Q = distinct_matrix(nq_pad // 2, ld)
        Q = np.concatenate([Q, -Q])
    else:
        Q = distinct_matrix(nq_pad, ld)
    qb = ref.bf16_bits(Q)
    for image, written in ((ref.q_image(Q, ld, nq_pad), nq_pad * ld), (ref.q_image16(Q, ld, nq_pad), nq_pad * ld)):
        assert image.size == (ld // 32) * 16 * 1024 // 2
        body = image[image != ref.SENTINEL16]
        values = qb.ravel()[qb.ravel() != ref.SENTINEL16]  # (at most one element shares the sentinel's bits)
        assert written - values.size <= 1 and np.array_equal(np.sort(body), np.sort(values))
    qt = nq_pad // 32
    img = ref.q_image(Q, ld, nq_pad)
    # K2b: chunk c = 1, tile t = 1, step s = 1, lane 32 h + r = 32 + 5, element 3 <- Q[32 + 5][32 + 16 + 8 + 3]
    assert img[(((1 * qt + 1) * 2 + 1) * 64 + 37) * 8 + 3] == qb[37, 59]
    img = ref.q_image16(Q, ld, nq_pad)
    # K2s: chunk 1, query tile 2, lane 16 g + r = 16 * 3 + 7, element 6 <- Q[32 + 7][32 + 24 + 6]
    assert img[((1 * (nq_pad // 16) + 2) * 64 + 55) * 8 + 6] == qb[39, 62]


def test_shadow_image_is_a_permutation_with_zero_padding_rows():
    ld, n, rows_img = 128, 100, 256
    X = distinct_matrix(n, ld)
    img = ref.shadow_image(X, n, rows_img, ld)
    assert img.size == rows_img * ld
    assert np.array_equal(np.sort(img[img != 0]), np.sort(ref.bf16_bits(X).ravel()))
    # rows 100 .. 255 are zero; row 37, column 77 sits in KiB (37 / 16) * 4 + 77 / 32 at [(77 / 8) % 4][37 % 16][77 % 8]
    row, col = np.meshgrid(np.arange(n, rows_img), np.arange(ld), indexing="ij")
    assert not img[ref.shadow_index(row, col, ld)].any()
    assert img[(2 * 4 + 2) * 512 + 1 * 128 + 5 * 8 + 5] == ref.bf16_bits(X)[37, 77]


def test_rank_largest_and_its_short_answers():
    v = np.array([3.0, -0.0, 0.0, -np.inf, 3.0, 7.5, -2.0], np.float32)
    assert [float(ref.rank_largest(v, r)) for r in (1, 2, 3, 4)] == [7.5, 3.0, 3.0, 0.0]
    assert np.signbit(ref.rank_largest(v, 5)) and ref.rank_largest(v, 5) == 0.0   # -0 ranks below +0
    assert ref.rank_largest(v, 7) == -np.inf
    assert ref.rank_largest(v, 9) == -np.inf and np.isnan(ref.rank_largest(v, 20, short="nan"))


@pytest.mark.parametrize("name", ref.CLASSES)
@pytest.mark.parametrize("l2", [False, True])
def test_a_plain_bf16_machine_stays_inside_the_margin(name, l2):
    for ld, d, n, nq in ((64, 64, 70, 8), (128, 100, 50, 6), (320, 320, 40, 5)):
        X, Q = ref.make_class(name, 11, n, nq, ld, d)
        qn, xn = ref.norms(Q), float(ref.norms(X).max())
        truth, rounded = ref.scores64(Q, X, l2), ref.scores64_rounded(Q, X, l2)
        m16 = ref.scores_f32_sequential(Q, X, l2, True).astype(np.float64)
        m32 = ref.scores_f32_sequential(Q, X, l2, False).astype(np.float64)
        assert np.isfinite(truth).all() and np.isfinite(m16).all() and np.isfinite(m32).all()
        for b in range(nq):
            rnd, acc, fl = ref.bf16_terms(l2, d, qn[b], xn)
            assert np.abs(rounded[b] - truth[b]).max() <= rnd + fl, (name, ld, b)
            assert np.abs(m16[b] - rounded[b]).max() <= acc + fl, (name, ld, b)
            assert np.abs(m16[b] - truth[b]).max() <= ref.eps(l2, True, d, qn[b], xn), (name, ld, b)
            assert np.abs(m32[b] - truth[b]).max() <= ref.eps(l2, False, d, qn[b], xn), (name, ld, b)
