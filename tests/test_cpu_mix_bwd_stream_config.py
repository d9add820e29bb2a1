"""The configuration row of the one-shot mix backward (csrc/config.hip: `sup_mix_stream` / MRGCN_SUP_MIX_STREAM)."""
import ctypes as C


def test_sup_mix_stream_is_a_described_row_that_round_trips():
    from mrgcn_amd import _lib
    lib = _lib.load()
    names = [lib.mrgcn_config_name(i).decode() for i in range(lib.mrgcn_config_count())]
    assert "sup_mix_stream" in names
    doc = lib.mrgcn_config_doc(names.index("sup_mix_stream"))
    assert doc and b"k_mix_bwd_stream" in doc and b"k_mix_bwd_sup" in doc
    v = C.c_int64(-1)
    assert lib.mrgcn_config_get(b"sup_mix_stream", C.byref(v)) == 0
    default = v.value
    assert default in (0, 1)
    try:
        for spelling, value in ((b"sup_mix_stream", 0), (b"MRGCN_SUP_MIX_STREAM", 1), (b"sup_mix_stream", 0)):
            assert lib.mrgcn_config_set(spelling, value) == 0
            assert lib.mrgcn_config_get(b"MRGCN_SUP_MIX_STREAM", C.byref(v)) == 0 and v.value == value
            assert _lib.config()["sup_mix_stream"] == value
    finally:
        assert lib.mrgcn_config_set(b"sup_mix_stream", default) == 0
    assert _lib.config()["sup_mix_stream"] == default
