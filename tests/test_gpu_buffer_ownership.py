"""Who frees the device buffers of the Python layer, with a failure injected at every allocation, every upload and every `*_dev` call of every
public entry point (distributed_plonk_amd/worker.py: DeviceScope).

A fresh PlonkWorker per curve has `alloc` and its `*_dev` methods wrapped on the instance and DeviceBuffer.upload patched: every buffer is
logged, and LIVE is the number of logged buffers whose `ptr` is set.  An entry of the table is (prepare, run): prepare makes the inputs
unobserved; run(w, state, own) calls the entry point, appends what the CALLER owns afterwards — a returned object with close(), a released
buffer, the BuiltCircuit it made — to `own` as soon as it has it, and returns how many buffers those document.  For each entry:

  (a) a clean run: at least one allocation, live = the documented count, 0 after closing `own`, and closing twice raises nothing;
  (b) the i-th allocation raises, for every i;   (c) the j-th upload raises, for every j;
  (d) each `*_dev` worker method the clean run called raises at its first call (the first of them is the entry's first library call);
  in (b) to (d) the injected exception itself comes out and, once `own` is closed, live = 0.

The failures are Python exceptions raised BEFORE the call into the library: the library never sees a bad pointer, size or freed buffer.
tests/test_hostemu_buffer_ownership.py runs all of it on the CPU emulation."""
import numpy as np
import pytest

from distributed_plonk_amd import builder as BD
from distributed_plonk_amd import circuit as CC
from distributed_plonk_amd import codec
from distributed_plonk_amd import edwards as ED
from distributed_plonk_amd import elgamal as EG
from distributed_plonk_amd import fr as _fr
from distributed_plonk_amd import rescue as RS
from distributed_plonk_amd import verifier as VF
from distributed_plonk_amd.synthetic import SyntheticInstance
from distributed_plonk_amd.transcript import serialize_fr, serialize_g1, serialize_proof
from distributed_plonk_amd.worker import DeviceBuffer, PlonkWorker
from tests.circuit_cases import TAU, prove_synthetic

pytestmark = pytest.mark.gpu

CIDS = {"bn254": 0, "bls12_381": 1}


class Injected(Exception):
    pass


class Tracker:
    """The observed worker.  `on`: calls are counted, logged and failed as reset() asked; off: everything passes through."""

    def __init__(self, w):
        self.w, self.bufs, self.on = w, [], False
        self.reset()
        real_alloc = w.alloc

        def alloc(nbytes):
            if not self.on:
                return real_alloc(nbytes)
            i, self.allocs = self.allocs, self.allocs + 1
            if i == self.fail_alloc:
                raise self.marker
            self.bufs.append(real_alloc(nbytes))
            return self.bufs[-1]

        w.alloc = alloc
        for name in dir(PlonkWorker):
            if name.endswith("_dev"):
                setattr(w, name, self._observed(name, getattr(w, name)))

    def _observed(self, name, real):
        def call(*a, **k):
            if self.on:
                self.calls.append(name)
                if name == self.fail_call:
                    raise self.marker
            return real(*a, **k)
        return call

    def upload(self, real, buf, arr):
        if self.on and buf.worker is self.w:
            j, self.uploads = self.uploads, self.uploads + 1
            if j == self.fail_upload:
                raise self.marker
        return real(buf, arr)

    def reset(self, alloc=None, upload=None, call=None):
        self.allocs = self.uploads = 0
        self.calls = []
        self.fail_alloc, self.fail_upload, self.fail_call = alloc, upload, call
        self.marker = Injected(f"alloc {alloc}, upload {upload}, call {call}")

    def live(self) -> int:
        return sum(1 for b in self.bufs if b.ptr)


@pytest.fixture(scope="module")
def trackers():
    made = {}
    real_upload = DeviceBuffer.upload

    def patched(buf, arr):
        t = next((t for t in made.values() if t.w is buf.worker), None)
        return t.upload(real_upload, buf, arr) if t else real_upload(buf, arr)

    def get(curve):
        if curve not in made:
            made[curve] = Tracker(PlonkWorker(me=0, device=0, curve=curve))
        return made[curve]

    DeviceBuffer.upload = patched
    try:
        yield get
    finally:
        DeviceBuffer.upload = real_upload
        for t in made.values():
            t.w.close()


def _close(o):
    o.close() if hasattr(o, "close") else o.free()


def exercise(t: Tracker, prepare, run, oracle, curve):
    scratch = []                                      # the caller's own device inputs of the *_dev entries: unobserved, freed at the end
    state = prepare(t.w, curve, oracle, lambda a: scratch.append(t.w.alloc(max(a.nbytes, 8)).upload(a)) or scratch[-1].ptr)

    def attempt(own, **fail):
        t.reset(**fail)
        t.on = True
        try:
            return run(t.w, state, own) or 0
        finally:
            t.on = False

    try:
        own = []
        documented = attempt(own)
        A, U, calls = t.allocs, t.uploads, list(dict.fromkeys(t.calls))
        assert A >= 1 and calls, "the entry allocated nothing through the observed worker, or called no *_dev method"
        assert t.live() == documented, f"clean run: {t.live()} live buffers, {documented} documented"
        for twice in range(2):
            for o in own:
                _close(o)
            assert t.live() == 0, "clean run: buffers live after close()"
        leaks = []                                    # every injection runs, whatever the ones before it left behind
        for kind, which in (("alloc", range(A)), ("upload", range(U)), ("call", calls)):
            for i in which:
                own = []
                with pytest.raises(Injected) as e:
                    attempt(own, **{kind: i})
                assert e.value is t.marker, (kind, i)
                for o in own:
                    _close(o)
                if t.live():
                    leaks.append(f"{kind} {i}: {t.live()} of {A}")
                    for b in t.bufs:                  # so that the next injection starts from nothing
                        b.free()
        assert not leaks, f"buffers stay allocated when these fail -> {leaks}"
    finally:
        for b in scratch:
            b.free()


# ---------------------------------------------------------------------------------------------- the table
ENTRIES = {}                                          # name -> (prepare(w, curve, oracle, scratch) -> state, run(w, state, own) -> documented, both curves?)


def entry(name, prepare, both_curves=True):
    def deco(run):
        ENTRIES[name] = (prepare, run, both_curves)
        return run
    return deco


def _limbs(curve, xs):
    return _fr.FIELDS[curve].vec_to_limbs([int(x) for x in xs])


def _g(curve):
    return VF.g1_generator(curve)


def _none(w, curve, oracle, scratch):
    return curve


def once_per_curve(prepare):
    """for inputs that hold no device memory: made by the first entry that needs them"""
    made = {}

    def cached(w, curve, oracle, scratch):
        if curve not in made:
            made[curve] = prepare(w, curve, oracle, scratch)
        return made[curve]
    return cached


# codec
@entry("codec.g1_from_bytes", _none)
def _(w, curve, own):
    xy, st = codec.g1_from_bytes(w, serialize_g1(curve, _g(curve), False) * 2)
    assert not st.any() and np.array_equal(xy[1], _g(curve))


@entry("codec.g1_to_bytes", _none)
def _(w, curve, own):
    assert codec.g1_to_bytes(w, np.stack([_g(curve)] * 2)) == serialize_g1(curve, _g(curve), False) * 2


@entry("codec.fr_from_bytes", _none)
def _(w, curve, own):
    x = _limbs(curve, [3, 4, 5])
    got, st = codec.fr_from_bytes(w, b"".join(serialize_fr(curve, l) for l in x))
    assert not st.any() and np.array_equal(got, x)


@entry("codec.fr_to_bytes", _none)
def _(w, curve, own):
    x = _limbs(curve, [3, 4, 5])
    assert codec.fr_to_bytes(w, x) == b"".join(serialize_fr(curve, l) for l in x)


@once_per_curve
def _proof_blob(w, curve, oracle, scratch):
    pt, ev = (_g(curve), False), list(_limbs(curve, range(1, 11)))
    return serialize_proof(curve, dict(wires_poly_comms=[pt] * 5, prod_perm_poly_comm=pt, split_quot_poly_comms=[pt] * 5, opening_proof=pt,
                                       shifted_opening_proof=pt, wires_evals=ev[:5], wire_sigma_evals=ev[5:9], perm_next_eval=ev[9]))


@entry("codec.proof_from_bytes", _proof_blob)
def _(w, blob, own):
    assert len(codec.proof_from_bytes(w, blob)["wires_evals"]) == 5


@entry("codec.proofs_from_bytes_dev", _proof_blob)
def _(w, blob, own):
    d_recs, status = codec.proofs_from_bytes_dev(w, [blob, blob])
    own.append(d_recs)
    assert not status.any()
    return 1


# rescue
@once_per_curve
def _rescue(w, curve, oracle, scratch):
    return RS.RescueParams.default(curve), _limbs(curve, range(10, 26))


@entry("rescue.permute", _rescue)
def _(w, s, own):
    assert RS.permute(w, s[0], s[1][:8].reshape(2, 4, 4)).shape == (2, 4, 4)


@entry("rescue.hash3", _rescue)
def _(w, s, own):
    assert RS.hash3(w, s[0], s[1][:6].reshape(2, 3, 4)).shape == (2, 4)


@entry("rescue.sponge", _rescue)
def _(w, s, own):
    assert RS.sponge(w, s[0], s[1][:4].reshape(2, 2, 4)).shape == (2, 1, 4)


@entry("rescue.stream", _rescue)
def _(w, s, own):
    assert RS.stream(w, s[0], s[1][4:6], s[1][:4].reshape(2, 2, 4)).shape == (2, 2, 4)


@entry("rescue.MerkleTree", _rescue, both_curves=False)
def _(w, s, own):
    own.append(RS.MerkleTree(w, s[0], s[1][:4]))
    return 1                                          # d_nodes


@entry("rescue.Accumulator+witness_inputs_dev", _rescue, both_curves=False)
def _(w, s, own):
    acc = RS.Accumulator(w, s[0], s[1][:4], 2)
    own.append(acc)
    own.append(acc.witness_inputs_dev([0, 3]))
    return 2 + 1                                      # d_elems, d_nodes; the released inputs


# edwards, elgamal
@once_per_curve
def _edwards(w, curve, oracle, scratch):
    prm = ED.EdwardsParams.default(curve)
    pts = np.stack([_limbs(curve, prm.mul_int(k, prm.generator)) for k in (3, 5)])
    sk, nonce, msg = _limbs(curve, [5, 9]), _limbs(curve, [77, 78]), _limbs(curve, [100, 101])
    pk = ED.keygen(w, prm, sk)
    texts = _limbs(curve, range(30, 34)).reshape(2, 2, 4)
    return dict(prm=prm, pts=pts, sc=_limbs(curve, [7, 11]), sk=sk, pk=pk, msg=msg, sigs=ED.schnorr_sign(w, prm, sk, nonce, msg), texts=texts,
                ct=EG.encrypt(w, prm, pk, texts, nonce))


@entry("edwards.mul", _edwards)
def _(w, s, own):
    assert ED.mul(w, s["prm"], s["sc"], s["pts"]).shape == (2, 2, 4)


@entry("edwards.fixed_mul", _edwards)
def _(w, s, own):
    assert np.array_equal(ED.fixed_mul(w, s["prm"], s["sk"]), s["pk"])


@entry("edwards.add", _edwards)
def _(w, s, own):
    assert ED.add(w, s["prm"], s["pts"], s["pts"][::-1]).shape == (2, 2, 4)


@entry("edwards.check", _edwards)
def _(w, s, own):
    assert (ED.check(w, s["prm"], s["pts"]) == (ED.ON_CURVE | ED.IN_SUBGROUP)).all()


@entry("edwards.schnorr_verify", _edwards)
def _(w, s, own):
    assert ED.schnorr_verify(w, s["prm"], s["pk"], s["msg"], s["sigs"]).all()


@entry("elgamal.dh_key", _edwards)
def _(w, s, own):
    assert EG.dh_key(w, s["prm"], s["sc"], s["pts"]).shape == (2, 4)


@entry("elgamal.encrypt", _edwards)
def _(w, s, own):
    E, ct = EG.encrypt(w, s["prm"], s["pk"], s["texts"], s["sc"])
    assert E.shape == (2, 2, 4) and ct.shape == (2, 2, 4)


@entry("elgamal.decrypt", _edwards)
def _(w, s, own):
    msg, ok = EG.decrypt(w, s["prm"], s["sk"], s["ct"])
    assert ok.all() and np.array_equal(msg, s["texts"])


# circuits: 8 gates, one of them hinted, so that the upload has its fourth buffer
def _built(curve):
    b = BD.CircuitBuilder(curve)
    x, y = b.input(2)
    out = b.public_input()
    b.enforce_equal(b.mul(b.pow5_lc([x, y], [1, 3], const=7), b.inv(y)), out)
    built = b.build()
    assert built.n == 8 and built.has_hints
    return built


def _circuit(w, curve, oracle, scratch):
    p = _fr.FIELDS[curve].p
    inputs, pub = _limbs(curve, [3, 5]), _limbs(curve, [(3 ** 5 + 3 * 5 ** 5 + 7) * pow(5, -1, p) % p])
    built = _built(curve)
    try:
        circ = built.circuit(w, inputs, pub)
    finally:
        built.close()
    padded = np.zeros((built.n, 4), np.uint64)
    padded[:1] = pub
    dev = dict(d_vars=scratch(circ.wire_vars), d_wit=scratch(circ.witness), d_sel=scratch(circ.selector_evals), d_pub=scratch(padded),
               d_inputs=scratch(np.concatenate([inputs, inputs])))
    return dict(curve=curve, inputs=inputs, pub=pub, circ=circ, n=built.n, num_vars=built.num_vars, **dev)


@entry("circuit.preprocess", _circuit)
def _(w, s, own):
    own.append(CC.preprocess(w, s["circ"]))
    return 7


@entry("circuit.preprocess_dev", _circuit, both_curves=False)
def _(w, s, own):
    own.append(CC.preprocess_dev(w, s["d_vars"], s["n"], s["num_vars"], s["d_wit"], s["d_sel"], s["d_pub"], 1))
    return 7                                          # d_wires, d_id, d_idx, d_sig_ev, d_sel, d_sig, d_pi


@entry("circuit.setup_dev+CircuitKey.instance", _circuit, both_curves=False)
def _(w, s, own):
    key = CC.setup_dev(w, s["d_vars"], s["n"], s["num_vars"], s["d_sel"], 1)
    own.insert(0, key)
    own.insert(0, key.instance(s["d_wit"], s["pub"]))
    return 5 + 2                                      # d_id, d_idx, d_sig_ev, d_sel, d_sig; the instance's d_wires, d_pi


UPLOAD = 4                                            # wire_vars, selector_evals, def_gate, hint_op


def _solve_entry(name, call, documented):
    @entry(name, _circuit)
    def _(w, s, own):
        built = _built(s["curve"])
        own.append(built)
        out = call(built, w, s)
        if hasattr(out, "close"):
            own.insert(0, out)
        return documented


_solve_entry("BuiltCircuit.solve_dev", lambda b, w, s: b.solve_dev(w, s["inputs"], s["pub"]), UPLOAD + 2)
_solve_entry("BuiltCircuit.solve_dev(d_inputs)", lambda b, w, s: b.solve_dev(w, None, s["pub"], d_inputs=s["d_inputs"]), UPLOAD + 1 + 2)
_solve_entry("BuiltCircuit.solve_many_dev", lambda b, w, s: b.solve_many_dev(w, np.stack([s["inputs"]] * 2), np.stack([s["pub"]] * 2)), UPLOAD + 1 + 2)
_solve_entry("BuiltCircuit.solve_many_dev(d_inputs)", lambda b, w, s: b.solve_many_dev(w, None, np.stack([s["pub"]] * 2), d_inputs=s["d_inputs"]),
             UPLOAD + 1 + 1 + 2)
_solve_entry("BuiltCircuit.preprocess", lambda b, w, s: b.preprocess(w, s["inputs"], s["pub"]), UPLOAD + 7)
_solve_entry("BuiltCircuit.circuit", lambda b, w, s: b.circuit(w, s["inputs"], s["pub"]), UPLOAD)


@entry("synthetic.SyntheticInstance", _none, both_curves=False)
def _(w, curve, own):
    own.append(SyntheticInstance(w, 3, tau=TAU))
    return 9                                          # d_wires, d_sel_ev, d_sig_ev, d_id, d_idx, d_pi, d_sel, d_sig, d_ck


# the verifier: two proofs of the smallest instance the verifier tests prove (tests/test_gpu_batch_verify_edges.py: LOG_N = 5)
@once_per_curve
def _proofs(w, curve, oracle, scratch):
    vk, pub, proofs = prove_synthetic(w, oracle, CIDS[curve], 5, 2, seed=11, num_inputs=1)
    return dict(vk=dict(vk, num_inputs=1), pub=[pub, pub], proofs=proofs, ok=VF.OpenKey.from_trapdoor(curve, TAU))


@entry("verifier.batch_verify", _proofs)
def _(w, s, own):
    assert VF.batch_verify(w, s["vk"], s["ok"], s["pub"], s["proofs"], seed=1) == [True, True]


@entry("verifier.batch_verify_multi", _proofs)
def _(w, s, own):
    assert VF.batch_verify_multi(w, [s["vk"]], s["ok"], [0, 0], s["pub"], s["proofs"], seed=1) == [True, True]


CASES = [(name, curve) for name, (_, _, both) in ENTRIES.items() for curve in (("bn254", "bls12_381") if both else ("bn254",))]


@pytest.mark.parametrize("name,curve", CASES, ids=[f"{n}-{c}" for n, c in CASES])
def test_every_exit_frees_what_the_call_owns(trackers, oracle, name, curve):
    prepare, run, _ = ENTRIES[name]
    exercise(trackers(curve), prepare, run, oracle, curve)
