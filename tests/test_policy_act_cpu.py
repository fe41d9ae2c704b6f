"""CPU: tmjx_policy_act / tmjx_policy_act_ok (csrc/tmjx_act.hip) are exported and validate their descriptor before any device call."""
import ctypes

from track_mjx_amd import hip


def _descriptor(**over):
    a = 1 << 20                                                    # a non-null, 16-byte aligned dummy address that is never dereferenced
    d = hip.PolicyAct()
    d.obs, d.ldo, d.mean, d.inv_std, d.nmean, d.nstd = a, 696, a, a, a, a
    d.n, d.K0, d.Z, d.obs_w, d.ref_w, d.A, d.n_enc, d.n_dec = 1365, 472, 60, 696, 470, 38, 2, 2
    for l in range(2):
        d.enc[l] = hip.DecoderBlock(a, a, a, a, 256, 472 if l == 0 else 256)
        d.dec[l] = hip.DecoderBlock(a, a, a, a, 256, 288 if l == 0 else 256)
    d.W2, d.b2, d.ldw2, d.Wh, d.bh, d.ldwh, d.ln_eps = a, a, 256, a, a, 256, 1e-6
    d.rng_state = a
    d.fc2 = d.logits = d.raw = d.action_t = d.logp = a
    for k, v in over.items():
        setattr(d, k, v)
    return d


def test_policy_act_validates_its_descriptor_without_gpu():
    L = hip.lib()
    a = 1 << 20
    assert L.tmjx_policy_act_ok(ctypes.byref(_descriptor())) == 1
    assert L.tmjx_policy_act_ok(ctypes.byref(_descriptor(eps=a, noise=a, rng_state=None))) == 1
    assert L.tmjx_policy_act_ok(ctypes.byref(_descriptor(mean=None, inv_std=None, nmean=None, nstd=None))) == 1
    assert L.tmjx_policy_act_ok(None) == 0 and L.tmjx_policy_act(None, None) == -22
    for bad, word in ((_descriptor(obs=None), b"null"), (_descriptor(logp=None), b"null"), (_descriptor(n=0), b">= 1"), (_descriptor(n_dec=0), b"blocks"),
                      (_descriptor(n_enc=5), b"blocks"), (_descriptor(Z=129), b"256"), (_descriptor(A=129), b"256"), (_descriptor(Z=63), b"288"),
                      (_descriptor(K0=470), b"K0"), (_descriptor(K0=476), b"K0"), (_descriptor(ldo=698), b"aligned"), (_descriptor(obs=a + 4), b"aligned"),
                      (_descriptor(ldo=692), b"ldo"), (_descriptor(inv_std=None), b"together"), (_descriptor(nstd=None), b"together"),
                      (_descriptor(ldw2=252), b"256"), (_descriptor(ldwh=1 << 21), b"1048576"), (_descriptor(Wh=a + 4), b"aligned"), (_descriptor(noise=a), b"together"),
                      (_descriptor(rng_state=None), b"rng_state"), (_descriptor(raw=a + 2), b"aligned")):
        assert L.tmjx_policy_act_ok(ctypes.byref(bad)) == 0
        assert L.tmjx_policy_act(ctypes.byref(bad), None) == -22 and word in L.tmjx_last_error(), (word, L.tmjx_last_error())
    for stack in ("enc", "dec"):
        for change, word in ((dict(width=64), b"256 wide"), (dict(width=512), b"256 wide"), (dict(gamma=None), b"null block"), (dict(W=a + 8), b"aligned"),
                             (dict(ldw=252), b"ldw")):
            d = _descriptor()
            for k, v in change.items():
                setattr(getattr(d, stack)[1], k, v)
            assert L.tmjx_policy_act_ok(ctypes.byref(d)) == 0
            assert L.tmjx_policy_act(ctypes.byref(d), None) == -22 and word in L.tmjx_last_error(), (stack, change, L.tmjx_last_error())
    d = _descriptor()
    d.dec[0].ldw = 284                                             # shorter than the decoder input rounded up to 4
    assert L.tmjx_policy_act(ctypes.byref(d), None) == -22 and b"ldw" in L.tmjx_last_error()
