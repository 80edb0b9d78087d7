"""GPU: enc_attn_kernel (launch_enc_attention through tools/bin/libnh_kref.so) on inputs that reach its deferred-maximum
rebase -- the rescale of O and l, the rewrite of the fp16 pair that subtracts m_ref inside the score product, the mixed ballot, p
up to 256, m_ref of either sign near 1100, a rebase inside the masked last tile -- against the fp64 reference of tests/kref.py.
Gaussian inputs (test_gpu_kernel_ref.py::test_enc_attention_matches_fp64) never rebase after tile 0; tests/test_kref_cpu.py pins
that down and checks cases, bound and mutations without a GPU.  kref.enc_rebase_case describes the four cases,
kref.enc_rebase_coverage what each must reach, kref.attn_bound the bound and its two terms for this kernel.
Out of scope: scores beyond +-60000 log2 units, where the kernel clamps -m_ref; the largest |m_ref| here is about 1300."""
import numpy as np
import pytest

import kref as K

pytestmark = pytest.mark.gpu

H = 2
WORST = {}      # worst |err| / bound per case, printed by each test (reported, never asserted)


def _enc_run(q, k, vt, B, S):
    """one launch_enc_attention with ldo = 2 d: `out` is [B*S][2][d] in memory and the kernel owns the even rows of d halfs;
    returns (the kernel's rows, the rows in between), the whole buffer filled with 7.25 beforehand"""
    d = 64 * H
    out = np.full((B * S, 2, d), np.float16(7.25), np.float16)
    rc = K.lib().kref_enc_attention(K.ptr(q), K.ptr(k), d, K.ptr(vt), K.ptr(out), 2 * d, B, S, H)
    K.check_rc(rc, f"enc attention B={B} S={S} H={H}")
    return out[:, 0], out[:, 1]


@pytest.mark.parametrize("B,S", K.ENC_REBASE_SHAPES)
@pytest.mark.parametrize("name", K.ENC_REBASE_CASES)
def test_enc_attention_rebase_cases_match_fp64(name, B, S):
    c = K.enc_rebase_reference(name, B, S, H)
    # before the GPU run: the bound catches the mask, the head slice and the four rebase bugs on this case's own data ...
    assert len(c["mutations"]) == 6
    caught = K.discriminates(c["ref"], c["bound"], c["mutations"])
    # ... and the inputs reach what the case is there for
    cov = K.enc_rebase_coverage(name, c["rep"], S)
    vt = K.vt_image(np.asarray(c["v"]), H, S)
    got, between = _enc_run(c["q"], c["k"], vt, B, S)
    WORST[name] = max(WORST.get(name, 0.0), K.violation(c["ref"], c["bound"], got))
    print(f"{name} B={B} S={S}: |err| / bound {K.violation(c['ref'], c['bound'], got):.3g} (worst so far {WORST[name]:.3g}); "
          f"coverage {cov}; mutations leave the bound by {({n: round(f, 1) for n, f in caught.items()})}")
    K.within(got, c["ref"], c["bound"], f"enc attention, {name} B={B} S={S}")
    assert np.all(between == np.float16(7.25)), "rows outside the launch were written"
    if name == "spike":
        # the pad rule where the rebase happens inside the masked tile: finite garbage in V^T columns S..1535 changes no bit
        vt2 = vt.copy()
        vt2[:, :, :, S:] = np.float16(1000.0)
        assert np.array_equal(_enc_run(c["q"], c["k"], vt2, B, S)[0].view(np.uint16), got.view(np.uint16))
