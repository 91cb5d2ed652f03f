"""tg_tcn_fwd_fused validates its arguments on the host before any launch: callable without a GPU (the style of tests/abi_fuzz.py, which
walks this entry point too through _lib.SIGNATURES)."""
import ctypes as C


def _call(lib, **over):
    scratch = (C.c_float * 4096)()                       # valid host memory, 16-byte aligned offsets below
    base = (C.addressof(scratch) + 15) // 16 * 16
    sp = C.c_void_p(base)
    biases = (C.c_void_p * 8)(*[base] * 8)
    a = dict(x0=sp, w_planes=sp, w_plane_stride=2401 * 608, w_rows=2400, w_inv=sp, biases=biases, dec_w=sp, dec_b=sp, rng_state=sp, site=1, p=0.3,
             clips=4, T=34, C=300, n_blocks=4, o0=sp, o1=sp, y=sp, save_row0=1, save_rows=2, out=sp, out_ld=32, stream=None)
    a.update(over)
    return lib.tg_tcn_fwd_fused(*a.values())


def test_fused_tcn_entry_point_refuses_bad_arguments(pkg):
    lib = pkg._lib.load()
    bad = [dict(x0=None), dict(w_planes=None), dict(w_inv=None), dict(biases=None), dict(dec_w=None), dict(dec_b=None), dict(out=None),
           dict(clips=0), dict(clips=-1), dict(T=12), dict(C=304), dict(n_blocks=3), dict(w_rows=2399), dict(w_plane_stride=2401 * 600),
           dict(p=1.0), dict(p=-0.1), dict(rng_state=None), dict(save_row0=-1), dict(save_row0=3, save_rows=2), dict(save_rows=-1),
           dict(o0=None), dict(y=None), dict(out_ld=31), dict(biases=(C.c_void_p * 8)()),
           dict(x0=C.c_void_p(C.addressof((C.c_float * 8)()) | 4))]
    for over in bad:
        rc = _call(lib, **over)
        assert rc != 0 and b"tg_tcn_fwd_fused" in lib.tg_last_error(), over
    # the bf16 tier keeps the conv-by-conv path
    assert lib.tg_set_math_mode(1) == 0
    try:
        assert _call(lib) != 0 and b"envelope" in lib.tg_last_error()
    finally:
        assert lib.tg_set_math_mode(0) == 0


def test_predicate_needs_planes_and_reads_the_switch(pkg):
    import torch
    ops = pkg.ops
    x0 = torch.zeros(2, 34, 300)
    assert isinstance(ops.TCN_FUSED, bool) and "T = 34" in ops.TCN_FUSED_ENVELOPE
    assert not ops.tcn_fused_takes(x0, None, 2, 4, torch.zeros(32, 300))
