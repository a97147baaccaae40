"""Optional legs of an N > 1 run (and of its one-GPU diagnostics --multi-path / --simulate-ranks), all AFTER and OUTSIDE the timed region:
the other distribution scheme, polynomial-level parallelism ("report both"), the verification of the distributed code path
against single-rank recomputation — and ClassProof, the five prover rounds with the coset-class prover that the N > 1 headline times.  Every function returns the dict that goes into
the line (every rank executes it: the legs contain collectives); bench.py stores it on rank 0."""
import os
import threading
import time

from .common import N_MSM, POLY_OP_COST, poly_parallel_assignment

TAU_SEED = 0x2F0D5EED0C0FFEE0123456789ABCDEF0FEDCBA98765432100F1E2D3C4B5A697      # the trapdoor a run publishes (mod p)


def other_scheme(b):
    """N > 1: the OTHER scheme, two steps after one warm-up, outside `value` (both are always visible in one SCALE run)"""
    other = b.step_ref2d if b.scheme == "classes" else b.step_classes
    other()
    b.full_sync()
    t1 = time.perf_counter()
    for _ in range(2):
        other()
    b.full_sync()
    dt2 = b.max_over_ranks(time.perf_counter() - t1)
    return {"scheme": "reference2d" if b.scheme == "classes" else "classes", "steps": 2, "ms_per_step": round(dt2 / 2 * 1e3, 3),
            "constraints_per_s": round(b.n / (dt2 / 2), 1),
            "note": "reference2d = all 33 transforms as the reference's 2-D distributed transform (33 RCCL all-to-alls per step; the 25 "
                    "forward coset FFTs take zero-padded rows, plonk_fft1_dev_compact, unless --dense-coset); classes = rank-local "
                    "coset classes, 2 data-path collectives per step"}


class _PolyParallel:
    """Polynomial-level parallelism ("Alternative for N that fits one GPU: polynomial-level parallelism ... zero communication -
    report both").  The 46 operations of a step are independent objects: every rank holds the whole SRS (1 GiB at 2^24; the reference
    replicates it too, dispatcher.rs:213-216) and takes WHOLE operations of the single-GPU step (poly_parallel_assignment: longest-processing-
    time-first) on the single-GPU step's own inputs, so the union over the ranks IS the single-GPU step.  No data-path collective; the 13
    commitments reach rank 0 in one 1.2 KiB all-gather (the varMsm replies).  --simulate-ranks S: the most loaded rank's share on one GPU."""

    def __init__(self, b):
        from distributed_plonk_amd import fr as _frp
        from distributed_plonk_amd.worker import PlonkWorker
        self.b = b
        args, n, m = b.args, b.n, b.m
        self.fp = _frp.FIELDS[args.curve]
        self.mine_all, self.load = poly_parallel_assignment(b.S, b.nbig)
        self.me = max(range(b.S), key=lambda r_: self.load[r_]) if b.sim else b.rank
        my_ops = self.mine_all[self.me]
        self.owner = {op: r_ for r_, ops_ in enumerate(self.mine_all) for op in ops_}
        self.c_idx = [i for k_, i in my_ops if k_ == "commit"]
        self.f_idx = [i for k_, i in my_ops if k_ == "coset_fft_8n"]
        self.s_idx = [i for k_, i in my_ops if k_ == "intt_n"]
        self.has_inv = ("coset_ifft_8n", 0) in my_ops
        self.bufs = []
        self.pw = [PlonkWorker(me=b.rank, device=b.local_rank, curve=args.curve) for _ in range(2)]
        for k_, v_ in b.experiment_opts.items():
            for x in self.pw:
                x.set_option(k_, v_)
        pw0 = self.pw[0]
        self.gen = self.fp.to_limbs(self.fp.generator)
        self.tiled = 0 if args.bases == "distinct" else min(n, 1 << 11)
        bases_full = self.alloc(n * 16 * b.q64)
        pw0.synth_bases(0x5EED, self.tiled, n, bases_full.ptr)                 # the single-GPU run's SRS, on every rank
        for x in self.pw:
            x.init_dev(bases_full.ptr, n, n, m)
            x.sync()
        self.scal, self.poly, self.small = {}, {}, {}
        for i in self.c_idx:
            self.scal[i] = self.alloc(n * 32)
            pw0.synth_fr(0x5CA1A5 + i, self.scal[i].ptr, n)
        for i in self.f_idx:
            self.poly[i] = self.alloc(b.poly_len * 32)
            pw0.synth_fr(0xC0EFF + i, self.poly[i].ptr, b.poly_len)
        for i in self.s_idx:
            self.small[i] = [self.alloc(n * 32), self.alloc(n * 32)]
            pw0.synth_fr(0xD15EA5E + i, self.small[i][0].ptr, n)
        self.out_m = self.alloc(m * 32) if self.f_idx else None
        self.inv_m = [self.alloc(m * 32), self.alloc(m * 32)] if self.has_inv else None
        if self.has_inv:
            pw0.synth_fr(0xBADC0DE, self.inv_m[0].ptr, m)
        pw0.sync()

    def alloc(self, nbytes):
        self.bufs.append(self.pw[0].alloc(nbytes))
        return self.bufs[-1]

    def step(self):
        from distributed_plonk_amd.dispatcher import gather_points
        b, pw, np = self.b, self.pw, self.b.np
        n, m, q64 = b.n, b.m, b.q64
        for i in self.s_idx:
            pair = self.small[i]
            pw[0].ntt_dev(pair[0].ptr, pair[1].ptr, n, True, False)
            pair[0], pair[1] = pair[1], pair[0]
        for i in self.f_idx:
            pw[0].coset_eval_dev(self.poly[i].ptr, b.poly_len, m, self.gen, self.out_m.ptr)
        if self.has_inv:
            pw[0].ntt_dev(self.inv_m[0].ptr, self.inv_m[1].ptr, m, True, True)
            self.inv_m[0], self.inv_m[1] = self.inv_m[1], self.inv_m[0]
        pw[0].sync()
        parts, errs = {}, []

        def run(lane):
            try:
                mine_c = self.c_idx[lane::2]
                if mine_c:
                    pts = pw[lane].commit_many_dev([(self.scal[i].ptr, n) for i in mine_c])
                    for j, i in enumerate(mine_c):
                        parts[i] = pts[j]
            except BaseException as ex_:     # noqa: BLE001 - re-raised below
                errs.append(ex_)

        th = [threading.Thread(target=run, args=(lane,)) for lane in range(2)]
        for t_ in th:
            t_.start()
        for t_ in th:
            t_.join()
        if errs:
            raise errs[0]
        table = np.zeros((N_MSM, 3 * q64), dtype=np.uint64)
        for i, pt in parts.items():
            table[i] = pt
        if b.sim:
            return table
        flat = table.reshape(-1)
        gathered = list(b.w.comm_allgather_host(flat, b.world)) if b.transport == "rccl" else gather_points(flat, None, b.dev)
        return np.stack([np.asarray(gathered[self.owner[("commit", i)]]).reshape(N_MSM, 3 * q64)[i] for i in range(N_MSM)])

    def sync(self):
        for x in self.pw:
            x.sync()
        self.b.dev_sync()
        if self.b.world > 1:
            self.b.dist.barrier()

    def verify(self, commits_tab):
        b, pw, np, fp_ = self.b, self.pw, self.b.np, self.fp
        n, m = b.n, b.m
        pv_ = {}
        # (a) a forward coset FFT of this rank: sampled outputs against Horner evaluations by an unrelated kernel
        ok = True
        if self.f_idx:
            i0 = self.f_idx[0]
            w_m_ = fp_.root_of_unity(m)
            pw[0].coset_eval_dev(self.poly[i0].ptr, b.poly_len, m, self.gen, self.out_m.ptr)
            for k2 in (0, 1, 9, (12345 + i0) % m, m - 1):
                x_ = fp_.to_limbs(fp_.generator * pow(w_m_, k2, fp_.p) % fp_.p)
                ok &= bool(np.array_equal(self.out_m.download((1, 4), byte_offset=k2 * 32)[0], pw[0].poly_eval_dev(self.poly[i0].ptr, b.poly_len, x_)))
        pv_["coset_fft_samples_vs_poly_eval_on_every_rank"] = b.every_rank(ok)
        # (b) a commitment of this rank: the batched launch set against the single-MSM path on the other context
        ok = True
        if self.c_idx:
            a_, ai = pw[0].g1_to_affine(commits_tab[self.c_idx[0]])
            b_, bi = pw[1].g1_to_affine(pw[1].commit_dev(self.scal[self.c_idx[0]].ptr, n))
            ok = bool(ai == bi and np.array_equal(a_, b_))
        pv_["commitment_batched_vs_single_msm_on_every_rank"] = b.every_rank(ok)
        # (c) rank 0 recomputes a commitment that ANOTHER rank produced and compares it with what the gather delivered
        ok = ok_exact = True
        if not b.sim and b.world > 1 and b.rank == 0:
            j = next(i for i in range(N_MSM - 1, -1, -1) if self.owner[("commit", i)] != 0)
            tmp = self.alloc(n * 32)
            pw[0].synth_fr(0x5CA1A5 + j, tmp.ptr, n)
            a_, ai = pw[0].g1_to_affine(commits_tab[j])
            b_, bi = pw[0].g1_to_affine(pw[0].commit_dev(tmp.ptr, n))
            ok = bool(ai == bi and np.array_equal(a_, b_))
            # ... and against the exact expected point from the CPU oracle (small MSMs of the aggregated scalars, oracle/checks.py)
            from oracle import checks as _chk, oracle as _O
            cid_ = _O.CURVE_IDS[b.args.curve]
            sc_ = _O.from_mont(cid_, tmp.download((n, 4)))
            want_ = _chk.msm_expected_distinct(cid_, 0x5EED, sc_) if b.args.bases == "distinct" else _chk.msm_expected_tiled(cid_, 0x5EED, self.tiled, sc_)
            e_, ei = _O.jac_to_affine(cid_, want_)
            ok_exact = bool(ai == ei and np.array_equal(a_, e_))
            del sc_
        if not b.sim and b.world > 1:
            pv_["gathered_commitment_of_another_rank_vs_recomputation_on_rank_0"] = b.every_rank(ok)
            pv_["gathered_commitment_of_another_rank_vs_oracle_exact"] = b.every_rank(ok_exact)
        return pv_

    def close(self):
        for buf in self.bufs:
            try:
                buf.free()
            except Exception:       # noqa: BLE001 - best-effort release of a diagnostic leg's buffers
                pass
        for x in self.pw:
            try:
                x.close()
            except Exception:       # noqa: BLE001
                pass


def polynomial_parallel(b):
    """two steps after one warm-up, outside `value`; verified on every rank unless --no-verify"""
    pp = None
    try:
        pp = _PolyParallel(b)
        pp.step()
        pp.sync()
        t1 = time.perf_counter()
        for _ in range(2):
            commits_tab = pp.step()
        pp.sync()
        dt3 = b.max_over_ranks(time.perf_counter() - t1)
        pv_ = pp.verify(commits_tab) if not b.args.no_verify else {}
        res = {"scheme": "polynomial_parallel", "steps": 2, "ms_per_step": round(dt3 / 2 * 1e3, 3), "constraints_per_s": round(b.n / (dt3 / 2), 1),
               "ranks": b.S, "operations_per_rank": [{k_: sum(1 for o in ops_ if o[0] == k_) for k_ in POLY_OP_COST} for ops_ in pp.mine_all],
               "modelled_load_ms_per_rank": [round(x, 1) for x in pp.load],
               "data_path_collectives_per_step": 0, "result_collectives_per_step": 0 if b.sim else 1,
               "verified": (bool(pv_) and all(pv_.values())) if not b.args.no_verify else None, "verification": pv_ or None,
               "note": "whole operations per rank (longest-processing-time-first over the step's 13 commitments, 25 zero-padded 8n coset FFTs, "
                       "the 8n coset iFFT and 7 size-n iNTTs), the whole SRS on every rank, the single-GPU step's inputs; the only collective "
                       "is the 1.2 KiB all-gather that brings the 13 commitments to rank 0"
                       + (f"; SIMULATED: the most loaded rank ({pp.me}) of {b.S} on one GPU" if b.sim else "")}
        if b.emulated:
            res.update(ms_per_step=None, constraints_per_s=None, modelled_load_ms_per_rank=None)
        return res
    finally:
        if pp is not None:
            pp.close()


def verify_multi(b):
    """N > 1 (and --multi-path): the distributed code path that was just timed, checked on every rank against a single-rank
    recomputation with the whole-vector path (which tests/ and the N = 1 run check against the oracle): one size-n inverse transform
    and one zero-padded 8n coset FFT through row pass -> RCCL all-to-all -> column pass, and a sharded commitment through the point
    all-gather.  -> the `verification` dict."""
    from distributed_plonk_amd import fr as _fr2
    from distributed_plonk_amd.dispatcher import _DevPtr, split_rc
    from distributed_plonk_amd.worker import PlonkWorker
    args, np, torch, w, n, m, S, rank = b.args, b.np, b.torch, b.w, b.n, b.m, b.S, b.rank
    n_loc, m_loc, q64, world = b.n_loc, b.m_loc, b.q64, b.world
    mv, tmp_bufs = {}, []

    def dev_i64(ptr, nbytes):
        if b.emulated:                      # "device" memory of the emulation is host memory
            import ctypes
            return torch.frombuffer((ctypes.c_char * nbytes).from_address(ptr), dtype=torch.int64)
        return torch.as_tensor(_DevPtr(ptr, nbytes), device=b.dev)

    def talloc(nbytes):
        tmp_bufs.append(w.alloc(nbytes))
        return tmp_bufs[-1]

    # (a) iNTT of size n: X[j*r + b] -> this rank's decimated rows are rows of the transposed [c][r] matrix
    r_n, c_n = split_rc(n)
    full, ref, rowsT, outn = talloc(n * 32), talloc(n * 32), talloc(n * 32), talloc(n_loc * 32)
    w.synth_fr(0x7E57, full.ptr, n)                                   # the same whole vector on every rank
    w.transpose_dev(full.ptr, rowsT.ptr, c_n, r_n)
    b.provers[0].fft_dev(rowsT.ptr + rank * (r_n // S) * c_n * 32, outn.ptr, n, False, True, False, out_layout=1)
    w.ntt_dev(full.ptr, ref.ptr, n, True, False)
    w.sync()
    b.dev_sync()
    got = dev_i64(outn.ptr, n_loc * 32).view(r_n, c_n // S, 4)
    want = dev_i64(ref.ptr, n * 32).view(r_n, c_n, 4)[:, rank * (c_n // S):(rank + 1) * (c_n // S), :]
    mv["distributed_intt_n_vs_single_rank_every_element"] = b.every_rank(torch.equal(got, want))
    if b.nbig:
        # (b) the zero-padded 8n coset FFT from compact rows (plonk_fft1_dev_compact) vs plonk_coset_eval_dev of the whole polynomial
        f2 = _fr2.FIELDS[args.curve]
        r_m, c_m = split_rc(m)
        L = (b.poly_len + r_m - 1) // r_m
        p_pad, rows_m, refm = talloc(r_m * L * 32), talloc(r_m * L * 32), talloc(m * 32)
        w.memset_dev(p_pad.ptr, 0, r_m * L * 32)
        w.synth_fr(0x7E58, p_pad.ptr, b.poly_len)
        w.transpose_dev(p_pad.ptr, rows_m.ptr, L, r_m)                # [L][r_m] -> [r_m][L]: row b = coefficients b, b + r_m, ...
        outm = b.buf_m[0][1]
        b.provers[0].fft_dev(rows_m.ptr + rank * (r_m // S) * L * 32, outm.ptr, m, True, False, True, out_layout=1, row_len=L)
        w.coset_eval_dev(p_pad.ptr, b.poly_len, m, f2.to_limbs(f2.generator), refm.ptr)
        w.sync()
        b.dev_sync()
        got = dev_i64(outm.ptr, m_loc * 32).view(r_m, c_m // S, 4)
        want = dev_i64(refm.ptr, m * 32).view(r_m, c_m, 4)[:, rank * (c_m // S):(rank + 1) * (c_m // S), :]
        mv["distributed_zero_padded_coset_fft_8n_vs_single_rank_every_element"] = b.every_rank(torch.equal(got, want))
    # (c) a round of two sharded commitments through the point all-gather vs every shard recomputed on THIS rank
    got_pt = w.g1_to_affine(b.commits_finish(b.commits_start(2)))
    chk = PlonkWorker(me=rank, device=b.local_rank, curve=args.curve)
    try:
        tb, ts = talloc(n_loc * 16 * q64), talloc(n_loc * 32)
        acc = None
        for r_ in range(world):
            chk.synth_bases(0x5EED + r_, 0 if args.bases == "distinct" else min(n_loc, 1 << 11), n_loc, tb.ptr)
            chk.init_dev(tb.ptr, n_loc, 0, 0)
            chk.synth_fr(0x5CA1A5 + 64 * r_ + (1 % len(b.scal)), ts.ptr, n_loc)
            part = chk.commit_dev(ts.ptr, n_loc)
            acc = part if acc is None else chk.g1_add(acc, part)
        want_pt = chk.g1_to_affine(acc)
    finally:
        chk.close()
    mv["sharded_commitment_vs_all_shards_on_one_rank"] = b.every_rank(want_pt[1] == got_pt[1] and np.array_equal(want_pt[0], got_pt[0]))
    for buf in tmp_bufs:
        buf.free()
    return mv


CLASS_FFT_HELPER_DEFAULT = "1"        # rank 0 of 8 simulated, same lease: 123.0 / 124.1 -> 114.8 / 115.3 ms per proof (profiles/r05_sim8_measurements.txt)


class _SimComm:
    """rank 0 of `size` ranks with nobody else there (diagnostic timing only): host objects come back `size` times; device collectives are the
    bench's stand-ins (Bench.sim_alltoall / sim_allgather: the bytes they would move, copied device to device on the worker's stream; nothing
    with --sim-exchange none)"""
    rank = 0

    def __init__(self, size, b, w):
        self.size, self.b, self.w = size, b, w
        self.bytes_out = 0
        # --sim-exchange none: the UNTIMED first proof still moves the stand-in's bytes, so that the receive buffers (named work buffers, reused
        # by the timed proof) hold field elements and not the zeros of a fresh allocation — round 4's 125.3 ms "rank 0 of 8" proof had committed
        # an all-zero quotient (4.3 ms for five 2^21-point commitments that cost 16.8 ms on data) and is void for that reason
        self.fill = True

    def all_gather_host(self, obj):
        return [obj] * self.size

    def all_to_all_dev(self, d_send, d_recv, nbytes):
        self.bytes_out += (self.size - 1) * nbytes
        self.b.sim_alltoall(self.w, d_send, d_recv, nbytes, force=self.fill)

    def all_gather_dev(self, d_send, d_recv, nbytes):
        self.bytes_out += (self.size - 1) * nbytes
        self.b.sim_allgather(self.w, d_send, d_recv, nbytes, force=self.fill)


class ClassProof:
    """The run's REAL proof on ALL ranks (N > 1, and its one-GPU diagnostics): the five prover rounds with the coset-class decomposition
    (class_prover.py) — the same satisfied synthetic instance on every rank (generated in HBM from the seed), the commit key sharded over the
    ranks (dispatcher2.rs:260-266), real transcript on every rank, degree check on.  `prove()` is one proof; bench.py times W + K of them as the
    headline of an N > 1 run and rank 0 hands the last one to the trapdoor verifier (`finish`).
    --simulate-ranks S: rank 0's share of an S-rank proof on ONE GPU with stand-in collectives (garbage proof, one rank's time)."""

    def __init__(self, b):
        from distributed_plonk_amd.class_prover import ClassProver, LibComm, TorchComm, key_shard_range
        from distributed_plonk_amd.synthetic import SyntheticInstance
        args, np, dist, w, n, m, sim, world = b.args, b.np, b.dist, b.w, b.n, b.m, b.sim, b.world
        self.b = b
        b.release_step_buffers()
        for x in set(b.workers) | set(b._extra_contexts()):      # the op-mix legs' caches (six pooled exchange buffers and the factor planes per context:
            x.trim()                                             # ~100 GiB on the one GPU of a --multi-path run at 2^24) go before the proof's buffers come
        if world == 1 and not dist.is_initialized() and not sim:
            os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
            os.environ.setdefault("MASTER_PORT", "29653")
            dist.init_process_group(rank=0, world_size=1, **b.pg_kwargs)
        fld = __import__("distributed_plonk_amd.fr", fromlist=["FIELDS"]).FIELDS[args.curve]
        self.TAU = TAU_SEED % fld.p
        self.G, r_ = (sim, 0) if sim else (world, b.rank)
        self.inst = inst = SyntheticInstance(w, args.log_n, seed=0xC1AC, num_inputs=3, tau=self.TAU, init_worker=False)
        self.key_range = klo, khi = key_shard_range(inst.key_size, r_, self.G)              # a rank KEEPS only its slice of the key
        for x in b.workers[:2]:
            x.init_dev(inst.d_ck.ptr + klo * 16 * b.q64, khi - klo, n, m)
        consts = np.arange(64, dtype=np.uint64).reshape(16, 4) + 11
        self.bl = {"wires": consts[5:15].reshape(5, 2, 4), "perm": consts[12:15]}
        if sim:
            self.comm = _SimComm(self.G, b, w)
        elif b.transport == "rccl" and b.multi:
            def _boot(obj):
                out_ = [None] * world
                dist.all_gather_object(out_, obj)
                return out_
            self.comm = LibComm(w, bootstrap=_boot)
        else:
            self.comm = TorchComm(w, None if b.emulated else b.dev)
        # the key's 18 class evaluations on a third context beside rounds 1-2 (ClassProver(fft_helper=...)): one of the step's transform contexts when the
        # run has them (--overlap-phases), PLONK_CLASS_FFT_HELPER=0 / 1 overrides the default
        want_helper = os.environ.get("PLONK_CLASS_FFT_HELPER", CLASS_FFT_HELPER_DEFAULT) == "1"
        self.fft_helper = b.step_workers[0] if (want_helper and b.step_workers) else None
        self.cp = ClassProver(w, args.log_n, self.comm, commit_helper=b.workers[1], key_range=(klo, khi), fft_helper=self.fft_helper)
        self.cp.load_key_dev(inst.sel_ptrs, inst.sig_ptrs, inst.k)
        self.pub = inst.public_inputs()
        self.vk = self.cp.verifying_key()                                                  # 18 sharded commitments, once per key
        self.proof = None
        self.n_proofs = 0
        # set-up, never timed: the first proof allocates the work buffers; under --sim-exchange none it still moves the stand-in's bytes so that the
        # receive buffers the later proofs reuse hold field elements and not the zeros of a fresh allocation (_SimComm.fill)
        self.prove()
        self.bytes_out_setup = self.comm.bytes_out if sim else 0

    def prove(self):
        cp, inst, b = self.cp, self.inst, self.b
        fs = cp.fiat_shamir(self.pub)
        if b.sim:
            self.comm.fill = self.n_proofs == 0
        self.proof = cp.prove_dev(inst.wev, inst.d_id.ptr, inst.d_idx.ptr, inst.d_pi.ptr, self.bl, fs, check_degree=not b.sim)
        self.n_proofs += 1
        return cp.timings

    @property
    def overlapped(self):
        return self.fft_helper is not None

    def close(self):
        """a run without --full: the timed proofs are all there is (finish() closes both itself)"""
        self.cp.close()
        self.inst.close()

    def finish(self, proof_ms, rounds_ms):
        """after the timed proofs: the resident-key variant, the verifier on rank 0 -> the row under next_rows.class_prover"""
        from distributed_plonk_amd.class_prover import ClassProver
        from distributed_plonk_amd.transcript import PlonkTranscript
        b, cp, inst, comm = self.b, self.cp, self.inst, self.comm
        args, np, n, sim = b.args, b.np, b.n, b.sim
        G_ = self.G
        bytes_out_per_proof = (comm.bytes_out - self.bytes_out_setup) // max(self.n_proofs - 1, 1) if sim else None
        r12 = "replicated (PLONK_CLASS_REPLICATED_R12=1 or one rank)" if cp.replicated_r12 else "size-n iFFTs by residue class, grand product by gate range"
        proof_c = self.proof
        cp.close()                                   # its work buffers (~150 GB at 2^24 on ONE rank) must go before the variant allocates its own
        # the same proof with this rank's class evaluations of the 18 proving-key polynomials resident (9.7 GB per rank at 2^24 / 8 ranks): a labelled
        # variant, like the single-GPU prover's resident_key_cosets — the reference re-transforms the key every proof
        t_res, same = None, None
        try:
            cpr = ClassProver(b.w, args.log_n, comm, commit_helper=b.workers[1], key_range=self.key_range, cache_key_cosets=True)
            cpr.load_key_dev(inst.sel_ptrs, inst.sig_ptrs, inst.k)
            cpr._key["vk"] = self.vk
            pr = None
            for it in range(2):
                fsr = cpr.fiat_shamir(self.pub)
                if sim:
                    comm.fill = it == 0
                b.full_sync()
                t0 = time.perf_counter()
                pr = cpr.prove_dev(inst.wev, inst.d_id.ptr, inst.d_idx.ptr, inst.d_pi.ptr, self.bl, fsr, check_degree=not sim)
                b.full_sync()
                t_res = (time.perf_counter() - t0) * 1e3
            t_res = b.max_over_ranks(t_res)
            same = None if sim else bool(all(np.array_equal(pr[k_][0], proof_c[k_][0]) for k_ in ("opening_proof", "shifted_opening_proof")))     # (a simulated rank proves garbage)
            cpr.close()
        except Exception as ex:     # noqa: BLE001 - a variant is a side note of a side leg
            t_res = None
            same = repr(ex)
        cverified = None
        if b.rank == 0 and not sim and not args.no_verify:
            try:
                from oracle import bigint_ref as B_, verifier_ref as V_
                V_.verify(B_.CURVES[args.curve], self.vk, self.pub, proof_c, self.TAU, transcript=PlonkTranscript(args.curve))
                cverified = True
            except Exception as ex:     # noqa: BLE001 - a rejected proof is a result, not a crash
                cverified = f"REJECTED: {ex!r}"
        row = {"n": n, "ranks": G_, "ms": None if proof_ms is None else round(proof_ms, 2),
               "constraints_per_s": None if proof_ms is None else round(n / proof_ms * 1e3, 1),
               "rounds_ms_rank0": rounds_ms,
               "variant_resident_key_class_cosets": {"ms": None if t_res is None else round(t_res, 2), "same_proof": same,
                                                     "note": "18 of the 25 class evaluations of round 3 kept in HBM across proofs; not the reference's work"},
               "accepted_by_verifier": cverified,
               "simulated": bool(sim),
               **({"sim_exchange": {"mode": args.sim_exchange, "device_bytes_out_per_proof": bytes_out_per_proof,
                                    "xgmi_model_ms_per_proof_at_153_GBps_per_link": round(bytes_out_per_proof / (G_ - 1) / 153e9 * 1e3, 2)}} if sim else {}),
               "rounds_1_2": r12,
               "key_class_evaluations": "on a third context beside rounds 1 and 2" if self.fft_helper is not None else "inside round 3",
               "collectives_per_proof": "1 all-to-all + 1 all-gather of quotient coefficients, 3 all-gathers of class values (the size-n iFFTs of rounds 1, 2, 3), "
                                        "1 all-gather of the product vector, 5 all-gathers of partial commitment points (one per round), "
                                        "5 all-gathers of 32-byte partials (slice totals + status, evaluations, degree, two openings)",
               "reference": "dispatcher2.rs:296-712 via distributed_plonk_amd/class_prover.py"}
        inst.close()
        return row
