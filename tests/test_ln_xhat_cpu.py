"""include/coati_ln_xhat.h without a GPU: the header is read like the others into a table of its own, the library exports its entries, and
the argument checks answer with codes before any HIP call."""
import ctypes

from coati_amd import _abi, _lib, build

ENTRIES = ["coati_engine_ln_saves_xhat", "coati_gemm_ln_gelu_grad", "coati_gemm_lnbwd_xhat", "coati_wgrad_grouped_affine"]


def test_header_is_a_table_of_its_own():
    assert sorted(_lib.LN_XHAT_PROTOTYPES) == ENTRIES
    for other in (_lib.PROTOTYPES, _lib.BEAM_PROTOTYPES, _lib.SEARCH_PROTOTYPES, _lib.GRAMMAR_PROTOTYPES, _lib.SCREEN_PROTOTYPES, _lib.GUIDE_PROTOTYPES):
        assert not set(ENTRIES) & set(other)
    assert not set(ENTRIES) & set(_lib.exported_symbols()) and _lib.ABI_VERSION == 5
    with open(build.HEADER) as f:
        base = _abi.parse(f.read())
    with open(build.LN_XHAT_HEADER) as f:
        again = _abi.parse(f.read(), guard="COATI_LN_XHAT_H", name="coati_ln_xhat.h", base=base)
    assert again.prototypes == _lib.LN_XHAT_PROTOTYPES and not again.experimental
    assert build.LN_XHAT_HEADER in build._sources()
    l = _lib.lib()
    for name in ENTRIES:
        assert hasattr(l, name), name


def test_gamma_beta_outside_256_wide_tiles_with_k_256_is_an_argument_error():
    l = _lib.lib()
    fake = 4096     # never dereferenced: the checks run on the host before any HIP call
    P1, L1, I1 = ctypes.c_void_p * 1, ctypes.c_int64 * 1, ctypes.c_int * 1
    def call(N, K, tile, gamma, beta):
        return l.coati_wgrad_grouped_affine(1, P1(fake), L1(N), P1(fake), L1(K), 37, I1(N), I1(K), P1(fake), L1(K), P1(fake),
                                            P1(gamma), P1(beta), tile, ctypes.c_void_p(fake), 1 << 20, None)
    assert call(768, 256, 128, fake, fake) == -1 and b"b_gamma" in l.coati_last_error()
    assert call(256, 512, 256, fake, fake) == -1 and b"b_gamma" in l.coati_last_error()
    assert call(768, 256, 256, fake, None) == -1 and b"come together" in l.coati_last_error()


def test_engine_reports_no_saved_xhat_before_any_forward():
    l = _lib.lib()
    cfg = _lib.CoatiConfig(2, 2, 64, 64, 64, 4, 24, 48, 5.0, 0, 1, 7, 0, 1, 1, 1, 1)
    h = ctypes.c_void_p()
    assert l.coati_engine_create(ctypes.byref(cfg), ctypes.byref(h)) == 0
    assert l.coati_engine_ln_saves_xhat(h, 0) == 0 and l.coati_engine_ln_saves_xhat(h, 1) == 0
    assert l.coati_engine_ln_saves_xhat(h, 2) == -1 and l.coati_engine_ln_saves_xhat(None, 0) == -1
    l.coati_engine_destroy(h)
