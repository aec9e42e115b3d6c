"""miden-vm_amd: host-side mirror of the reference's prover interface over libmidenhip's C ABI.

The reference's host language is Rust (no toolchain in this image), so this Python layer stands in
for the Rust shim in tests and benches; names follow the reference:
  commit_traces ............... crates/lifted-stark/src/prover/commit.rs:142-180
  Committed.root()/tree() ..... crates/lifted-stark/src/prover/commit.rs:60-77
  LmcsTree.prove_batch ........ crates/lifted-stark/src/lmcs/lifted_tree.rs:155-180
  coset_lde_batch ............. p3-dft call at prover/commit.rs:173
  Poseidon2Permutation256 ..... crates/crypto/src/hash/algebraic_sponge/poseidon2/mod.rs:340-386
There is NO CPU fallback: if libmidenhip.so or a GPU is missing, construction raises.
"""
import ctypes as C
import os
import weakref
import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("MIDENHIP_LIB") or os.path.join(_HERE, "lib", "libmidenhip.so")  # override: experiment builds only
P = 0xFFFFFFFF00000001
u64p = C.POINTER(C.c_uint64)

EXPORTS = [
    "mh_ctx_create", "mh_ctx_destroy", "mh_ctx_trim", "mh_ctx_mem_stats", "mh_last_error", "mh_device_count", "mh_prof_enable", "mh_prof_filter", "mh_prof_reset",
    "mh_prof_get", "mh_prof_dump", "mh_poseidon2_permute", "mh_poseidon2_register_rate", "mh_coset_lde_batch", "mh_trace_upload", "mh_trace_upload_async", "mh_trace_upload_cols_async", "mh_trace_wait", "mh_trace_free",
    "mh_commit_traces", "mh_tree_free", "mh_tree_root", "mh_tree_log_height", "mh_tree_open", "mh_tree_download_lde",
    "mh_tree_download_layers", "mh_air_load", "mh_air_free", "mh_air_log_quotient_degree", "mh_air_compiled_chunks", "mh_air_compiled_max_vgprs", "mh_jit_precompile", "mh_prove", "mh_prove_host", "mh_proof_free",
    "mh_proof_num_fields", "mh_proof_num_commitments", "mh_proof_fields", "mh_proof_commitments", "mh_proof_digest",
    "mh_proof_num_traces", "mh_proof_log_trace_heights", "mh_proof_serialize", "mh_shard_commit_leaves", "mh_shard_free",
    "mh_shard_leaf_digests", "mh_shard_build_subtree", "mh_merkle_cap_root", "mh_merkle_cap_root_lmcs", "mh_prove_sharded", "mh_commit_traces_sharded", "mh_trace_upload_sharded",
    "mh_session_begin", "mh_session_free", "mh_session_shape", "mh_session_commit_main", "mh_session_commit_aux",
    "mh_session_commit_quotient", "mh_session_ood_point_ok", "mh_session_ood", "mh_session_deep", "mh_session_fri_commit",
    "mh_session_fri_fold", "mh_session_fri_final", "mh_session_open", "mh_grind",
    "mh_host_alloc", "mh_host_free", "mh_verify", "mh_trace_from_device", "mh_lookup_load", "mh_lookup_free", "mh_air_attach_lookup", "mh_air_attach_preprocessed", "mh_lookup_build_aux", "mh_trace_download",
    "mh_verify_ex", "mh_external_logup_balance", "mh_external_precompile_session", "mh_external_precompile_session_ec_only", "mh_precompile_pcs_params", "mh_precompile_load", "mh_precompile_free",
    "mh_precompile_air_blob", "mh_precompile_preprocessed_root", "mh_precompile_pre_observe", "mh_prove_precompile", "mh_prove_precompile_traces", "mh_verify_precompile", "mh_proof_deserialize", "mh_ctx_set_lmcs", "mh_ctx_get_lmcs", "mh_blake3", "mh_verify_lmcs", "mh_grind_bytes",
    "mh_rccl_unique_id", "mh_comm_create_rccl", "mh_comm_destroy", "mh_comm_selftest",
    "mh_local_fabric_create", "mh_local_fabric_destroy", "mh_local_fabric_abort", "mh_comm_create_local",
    "mh_miden_load", "mh_miden_free", "mh_prove_miden", "mh_prove_miden_traces", "mh_verify_miden", "mh_miden_pcs_params",
    "mh_miden_challenger_state", "mh_miden_hash_kernel_digests", "mh_miden_pre_observe", "mh_miden_eval_external", "mh_miden_air_blob",
    "mh_check_constraints", "mh_constraint_fold", "mh_check_miden", "mh_check_miden_traces", "mh_check_precompile", "mh_check_precompile_traces",
    "mh_check_balance", "mh_check_balance_miden", "mh_check_balance_miden_traces", "mh_check_balance_precompile", "mh_check_balance_precompile_traces",
    "mh_fill_multiplicities", "mh_fill_multiplicities_miden_traces", "mh_fill_multiplicities_precompile_traces",
    "mh_poseidon2_trace_build", "mh_miden_poseidon2_trace", "mh_fill_range_table", "mh_fill_range_table_miden_traces",
    "mh_memory_section_build", "mh_miden_memory_section", "mh_memory_section_tile",
    "mh_hasher_section_build", "mh_miden_hasher_section", "mh_hasher_section_tile",
    "mh_bitwise_section_build", "mh_miden_bitwise_section", "mh_ace_section_build", "mh_miden_ace_section", "mh_ace_section_tile",
    "mh_kernel_rom_section_build", "mh_miden_kernel_rom_section", "mh_miden_chiplets_build", "mh_miden_chiplets_frame",
    "mh_keccak_round_program", "mh_keccak_round_levels", "mh_keccak_round_trace_build", "mh_keccak_traces_build",
    "mh_poseidon2_chiplet_plan", "mh_poseidon2_chiplet_trace_build", "mh_uint_traces_plan", "mh_uint_traces_build",
    "mh_ec_traces_plan", "mh_ec_traces_build",
    "mh_chunk_node_plan", "mh_chunk_node_trace_build", "mh_transcript_eval_plan", "mh_transcript_eval_trace_build",
    "mh_ctx_set_salt", "mh_ctx_get_salt", "mh_tree_salt_elems", "mh_tree_salt_index", "mh_tree_download_salt", "mh_verify_hiding",
    "mh_commit_host", "mh_precompile_setup_root",
    "mh_pcs_point_ok", "mh_pcs_begin", "mh_pcs_free", "mh_pcs_shape", "mh_pcs_evals", "mh_pcs_deep", "mh_pcs_download_deep", "mh_pcs_fri_commit",
    "mh_pcs_fri_fold", "mh_pcs_fri_final", "mh_pcs_query", "mh_pcs_open", "mh_pcs_verify", "mh_session_trees",
    "mh_lmcs_verify", "mh_lmcs_verify_batch", "mh_verify_batch", "mh_verify_miden_batch",
    "mh_lmcs_witness_size", "mh_lmcs_witness", "mh_lmcs_witness_batch", "mh_verify_batch_witness", "mh_witness_set_trees",
    "mh_witness_set_tree", "mh_witness_set_free", "mh_verify_miden_batch_witness",
]

MH_MAX_SALT_ELEMS = 8  # mh_ctx_set_salt: the largest salt width of the hiding LMCS
MH_PCS_MAX_POINTS = 4  # mh_pcs_*: the largest number of points one opening takes

# the in-tree cache of precompiled constraint kernels (filled by __graft_entry__.build() / tools/jit_precompile.py); $MH_JIT_CACHE_DIR wins
# It is consulted READ-ONLY ($MH_JIT_CACHE_RO_DIR): kernels this box has to compile itself (another hiprtc version, another AIR) go to
# the user's cache ($MH_JIT_CACHE_DIR, default ~/.cache/midenhip), never into the package directory.
_JIT_CACHE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "jit_cache")
if os.path.isdir(_JIT_CACHE):
    os.environ.setdefault("MH_JIT_CACHE_RO_DIR", _JIT_CACHE)

_lib = None


class MidenHipError(RuntimeError):
    pass


# ---- constraint checker (include/midenhip.h mh_check_*) ----
MH_ERR_UNSATISFIED = 6  # the trace does not satisfy the statement; the entries say where
MH_CHECK_EXACT = 1      # flags: evaluate every constraint on every row (no fold screen)


class CheckEntry(C.Structure):
    """mh_check_entry: a constraint of `instance` that does not vanish on `rows` rows, the first being `first_row` where it takes
    `value` (EF pair); instance -1 is an external (cross-AIR) assertion, `constraint` its index."""
    _fields_ = [("instance", C.c_int32), ("constraint", C.c_uint32), ("rows", C.c_uint64), ("first_row", C.c_uint64),
                ("value", C.c_uint64 * 2)]

    def key(self):
        return (self.instance, self.constraint, self.rows, self.first_row, self.value[0], self.value[1])

    def __eq__(self, other):
        return isinstance(other, CheckEntry) and self.key() == other.key()

    def __hash__(self):
        return hash(self.key())

    def __repr__(self):
        return (f"CheckEntry(instance={self.instance}, constraint={self.constraint}, rows={self.rows}, first_row={self.first_row}, "
                f"value=({self.value[0]}, {self.value[1]}))")


def _run_check(ctx, call, cap=256):
    """call(out, cap, n_ptr) -> rc; re-run with room for every entry when the first buffer was short."""
    while True:
        out, n = (CheckEntry * max(1, cap))(), C.c_size_t(0)
        rc = call(out, C.c_size_t(cap), C.byref(n))
        if rc not in (0, MH_ERR_UNSATISFIED):
            ctx.check(rc)
        if n.value <= cap:
            return [out[i] for i in range(n.value)]
        cap = n.value


# ---- bus balance (include/midenhip.h mh_check_balance*) ----
MH_BALANCE_NO_PUSHES = (1 << 64) - 1  # BalanceEntry.first_push: the push list was not collected (more than 2^22 pushes)


class BalancePush(C.Structure):
    """mh_balance_push: a live push (the reference's PushRecord without msg_repr); instance -1 is a boundary push of the statement."""
    _fields_ = [("instance", C.c_int32), ("column", C.c_uint32), ("fraction", C.c_uint32), ("row", C.c_uint64),
                ("multiplicity", C.c_uint64 * 2)]

    def key(self):
        return (self.instance, self.row, self.column, self.fraction, (self.multiplicity[0], self.multiplicity[1]))

    def __eq__(self, other):
        return isinstance(other, BalancePush) and self.key() == other.key()

    def __hash__(self):
        return hash(self.key())

    def __repr__(self):
        return (f"BalancePush(instance={self.instance}, row={self.row}, column={self.column}, fraction={self.fraction}, "
                f"multiplicity=({self.multiplicity[0]}, {self.multiplicity[1]}))")


class BalanceEntry(C.Structure):
    """mh_balance_entry: an encoded denominator whose net multiplicity is not zero (the reference's Unmatched).  `pushes` is the exact
    number of live pushes on it; `push_list` (set by check_balance) holds them, or None when the push list was not collected."""
    _fields_ = [("denom", C.c_uint64 * 2), ("net", C.c_uint64 * 2), ("pushes", C.c_uint64), ("first_push", C.c_uint64)]
    push_list = None

    def key(self):
        return ((self.denom[0], self.denom[1]), (self.net[0], self.net[1]), self.pushes, self.first_push)

    def __eq__(self, other):
        return isinstance(other, BalanceEntry) and self.key() == other.key() and self.push_list == other.push_list

    def __hash__(self):
        return hash(self.key())

    def __repr__(self):
        return (f"BalanceEntry(denom=({self.denom[0]}, {self.denom[1]}), net=({self.net[0]}, {self.net[1]}), pushes={self.pushes}, "
                f"first_push={self.first_push}, push_list={self.push_list})")


def _run_balance(ctx, call, entry_cap=256, push_cap=1024):
    """call(entries, entry_cap, n_entries_ptr, pushes, push_cap, n_pushes_ptr) -> rc; re-run with room for everything when a buffer was
    short.  -> [BalanceEntry], each with its push_list."""
    while True:
        ent, psh = (BalanceEntry * max(1, entry_cap))(), (BalancePush * max(1, push_cap))()
        ne, np_ = C.c_size_t(0), C.c_size_t(0)
        rc = call(ent, C.c_size_t(entry_cap), C.byref(ne), psh, C.c_size_t(push_cap), C.byref(np_))
        if rc not in (0, MH_ERR_UNSATISFIED):
            ctx.check(rc)
        collected = ne.value == 0 or ent[0].first_push != MH_BALANCE_NO_PUSHES
        if ne.value <= entry_cap and (np_.value <= push_cap or not collected):
            out = []
            for i in range(ne.value):
                e = BalanceEntry.from_buffer_copy(ent[i])
                e.push_list = [BalancePush.from_buffer_copy(psh[e.first_push + k]) for k in range(e.pushes)] if collected else None
                out.append(e)
            return out
        entry_cap, push_cap = max(entry_cap, ne.value), max(push_cap, np_.value if collected else 0)


def check_balance(ctx, lookups, traces, randomness, boundary=(), preprocessed=None, exact=False):
    """mh_check_balance: net the live pushes of the DeviceLookup programs `lookups` over `traces` (Trace objects or host matrices) under
    the challenges `randomness` (EF pairs), plus the boundary pushes `boundary` = [((c0, c1), +1 | -1)].  preprocessed: None, or per
    instance the raw preprocessed matrix (or None).  -> [BalanceEntry] ascending by denominator, each with its push_list; [] when the
    buses balance.  exact=True skips the sum screen."""
    lib = ctx.lib
    n = len(lookups)
    if len(traces) != n or (preprocessed is not None and len(preprocessed) != n):
        raise MidenHipError("check_balance: one trace (and one preprocessed matrix or None) per lookup program expected")
    tr = [_as_trace(ctx, t) for t in traces]
    pr = [_as_trace(ctx, t) for t in (preprocessed if preprocessed is not None else [None] * n)]
    la = (C.c_void_p * max(1, n))(*[l.h for l in lookups])
    ta = (C.c_void_p * max(1, n))(*[t.h for t in tr])
    pa = (C.c_void_p * max(1, n))(*[t.h if t is not None else None for t in pr])
    rnd = _arr([int(x) for r in randomness for x in r] or [0])
    bd = _arr([int(x) for d, _ in boundary for x in d] or [0])
    bs = np.ascontiguousarray([int(s) for _, s in boundary] or [0], dtype=np.int32)
    flags = C.c_int(MH_CHECK_EXACT if exact else 0)

    def call(ent, ecap, ne, psh, pcap, np_):
        return lib.mh_check_balance(ctx.h, C.c_int(n), la, ta, pa, _ptr(rnd), C.c_size_t(len(randomness)), _ptr(bd),
                                    bs.ctypes.data_as(C.POINTER(C.c_int32)), C.c_size_t(len(boundary)), flags, ent, ecap, ne, psh, pcap, np_)

    return _run_balance(ctx, call)


# ---- multiplicity columns (include/midenhip.h mh_fill_multiplicities*) ----
class MultSlot(C.Structure):
    """mh_mult_slot: fraction `fraction` of LogUp column `lookup_column` of instance `instance` has a multiplicity that is affine in
    main-trace column `main_column`."""
    _fields_ = [("instance", C.c_int32), ("lookup_column", C.c_uint32), ("fraction", C.c_uint32), ("main_column", C.c_uint32)]


def _slot_array(slots):
    """[(instance, lookup_column, fraction, main_column) | MultSlot] -> (ctypes array, count)"""
    sl = [s if isinstance(s, MultSlot) else MultSlot(*[int(x) for x in s]) for s in slots]
    return (MultSlot * max(1, len(sl)))(*sl), C.c_size_t(len(sl))


def _run_fill(ctx, call):
    """call(n_written_ptr, entries, ...) as _run_balance's: a second run (short buffers) finds the traces filled and writes the same."""
    written = C.c_uint64(0)
    report = _run_balance(ctx, lambda *out: call(C.byref(written), *out))
    return written.value, report


def fill_multiplicities(ctx, lookups, traces, slots, randomness, boundary=(), preprocessed=None):
    """mh_fill_multiplicities: fill the multiplicity cells the slots name, in place, in the device storage of `traces` (Trace objects),
    so that every key's net is zero; then the exact balance check.  slots: [(instance, lookup_column, fraction, main_column)];
    randomness / boundary / preprocessed as check_balance.  -> (cells written, [BalanceEntry]); [] when every bus balances."""
    lib = ctx.lib
    n = len(lookups)
    if len(traces) != n or (preprocessed is not None and len(preprocessed) != n):
        raise MidenHipError("fill_multiplicities: one trace (and one preprocessed matrix or None) per lookup program expected")
    if not all(isinstance(t, Trace) for t in traces):
        raise MidenHipError("fill_multiplicities: Trace objects expected (the traces are filled in place on the device)")
    pr = [_as_trace(ctx, t) for t in (preprocessed if preprocessed is not None else [None] * n)]
    la = (C.c_void_p * max(1, n))(*[l.h for l in lookups])
    ta = (C.c_void_p * max(1, n))(*[t.h for t in traces])
    pa = (C.c_void_p * max(1, n))(*[t.h if t is not None else None for t in pr])
    rnd = _arr([int(x) for r in randomness for x in r] or [0])
    bd = _arr([int(x) for d, _ in boundary for x in d] or [0])
    bs = np.ascontiguousarray([int(s) for _, s in boundary] or [0], dtype=np.int32)
    sa, ns = _slot_array(slots)

    def call(written, ent, ecap, ne, psh, pcap, np_):
        return lib.mh_fill_multiplicities(ctx.h, C.c_int(n), la, ta, pa, _ptr(rnd), C.c_size_t(len(randomness)), _ptr(bd),
                                          bs.ctypes.data_as(C.POINTER(C.c_int32)), C.c_size_t(len(boundary)), sa, ns, written, ent, ecap, ne,
                                          psh, pcap, np_)

    return _run_fill(ctx, call)


# ---- the range-check table (include/midenhip.h mh_fill_range_table*) ----
class RangeSlot(C.Structure):
    """mh_range_slot: fraction `fraction` of LogUp column `lookup_column` of instance `instance` is the range table's provider; its
    denominator encodes main-trace column `value_column`, its multiplicity is affine in `mult_column`."""
    _fields_ = [("instance", C.c_int32), ("lookup_column", C.c_uint32), ("fraction", C.c_uint32), ("value_column", C.c_uint32),
                ("mult_column", C.c_uint32)]


class RangeTableInfo(C.Structure):
    """mh_range_table_info: the table holds n_values distinct values in rows_needed rows (bridge rows and the trailing row included);
    the declaring trace has rows_available."""
    _fields_ = [("n_values", C.c_uint64), ("rows_needed", C.c_uint64), ("rows_available", C.c_uint64)]

    def __repr__(self):
        return f"RangeTableInfo(n_values={self.n_values}, rows_needed={self.rows_needed}, rows_available={self.rows_available})"


def _run_range(ctx, call, info):
    """_run_fill for a call that also fills `info`; a refusal carries it as `e.info`."""
    try:
        return _run_fill(ctx, call)[1], info
    except MidenHipError as e:
        e.info = info
        raise


def fill_range_table(ctx, lookups, traces, slot, randomness, boundary=(), preprocessed=None):
    """mh_fill_range_table: lay the range-check table of `slot` = (instance, lookup_column, fraction, value_column, mult_column) from
    the lookups of the statement, in place, in the device storage of `traces` (Trace objects): the value column and the multiplicity
    column are overwritten whatever they held.  randomness / boundary / preprocessed as check_balance.
    -> ([BalanceEntry], RangeTableInfo); [] when every bus balances.  A table that does not fit its trace, or a slot whose denominator
    is not uniform and affine in the value cell, raises MidenHipError with `e.info`; nothing was written then."""
    lib = ctx.lib
    n = len(lookups)
    if len(traces) != n or (preprocessed is not None and len(preprocessed) != n):
        raise MidenHipError("fill_range_table: one trace (and one preprocessed matrix or None) per lookup program expected")
    if not all(isinstance(t, Trace) for t in traces):
        raise MidenHipError("fill_range_table: Trace objects expected (the traces are filled in place on the device)")
    pr = [_as_trace(ctx, t) for t in (preprocessed if preprocessed is not None else [None] * n)]
    la = (C.c_void_p * max(1, n))(*[l.h for l in lookups])
    ta = (C.c_void_p * max(1, n))(*[t.h for t in traces])
    pa = (C.c_void_p * max(1, n))(*[t.h if t is not None else None for t in pr])
    rnd = _arr([int(x) for r in randomness for x in r] or [0])
    bd = _arr([int(x) for d, _ in boundary for x in d] or [0])
    bs = np.ascontiguousarray([int(s) for _, s in boundary] or [0], dtype=np.int32)
    sl = slot if isinstance(slot, RangeSlot) else RangeSlot(*[int(x) for x in slot])
    info = RangeTableInfo()

    def call(written, ent, ecap, ne, psh, pcap, np_):
        return lib.mh_fill_range_table(ctx.h, C.c_int(n), la, ta, pa, _ptr(rnd), C.c_size_t(len(randomness)), _ptr(bd),
                                       bs.ctypes.data_as(C.POINTER(C.c_int32)), C.c_size_t(len(boundary)), C.byref(sl), C.byref(info),
                                       written, ent, ecap, ne, psh, pcap, np_)

    return _run_range(ctx, call, info)


class P2TraceInfo(C.Structure):
    """mh_p2_trace_info: k = n_requests cycles carry a request, read from n_input_rows controller input rows (0: a host list); `defect`
    0 none, 1 id out of range, 2 id gap, 3 conflicting states for one id, 4 too many requests for log_n; `defect_row` the lowest
    chiplets row (1, 3) or id (2, 4)."""
    _fields_ = [("n_requests", C.c_uint64), ("n_input_rows", C.c_uint64), ("log_n", C.c_int32), ("defect", C.c_int32), ("defect_row", C.c_uint64)]

    def __repr__(self):
        return (f"P2TraceInfo(n_requests={self.n_requests}, n_input_rows={self.n_input_rows}, log_n={self.log_n}, defect={self.defect}, "
                f"defect_row={self.defect_row})")


def poseidon2_trace(ctx, states, multiplicities, log_n=None):
    """mh_poseidon2_trace_build: fill_poseidon2_permutation_trace on the device from a request list -- states [k, 12], multiplicities [k]
    (any uint64, reduced mod p) -> Trace [2^log_n, 16]; log_n None: max(6, ceil log2((k + 1) * 16)).  `Trace.p2_info` is the call's
    P2TraceInfo."""
    st = _arr(states).reshape(-1, 12)
    mu = _arr(multiplicities).reshape(-1)
    if mu.size != st.shape[0]:
        raise MidenHipError("poseidon2_trace: one multiplicity per state")
    lib = ctx.lib
    lib.mh_poseidon2_trace_build.argtypes = [C.c_void_p, u64p, u64p, C.c_size_t, C.c_int, C.POINTER(C.c_void_p), C.POINTER(P2TraceInfo)]
    h, info = C.c_void_p(), P2TraceInfo()
    ctx.check(lib.mh_poseidon2_trace_build(ctx.h, _ptr(st), _ptr(mu), st.shape[0], -1 if log_n is None else int(log_n), C.byref(h), C.byref(info)))
    t = Trace.from_handle(ctx, h, int(info.log_n), 16)
    t.p2_info = info
    return t


# ---- the memory chiplet's trace section (include/midenhip.h mh_memory_section_build, mh_miden_memory_section) ----
MEM_ACCESS_DTYPE = np.dtype([("ctx", "<u4"), ("addr", "<u4"), ("clk", "<u4"), ("kind", "<u4"), ("value", "<u8", (4,))])  # mh_mem_access
MEM_READ, MEM_WORD = 1, 2  # mh_mem_access.kind bits


class MemSectionInfo(C.Structure):
    """mh_mem_section_info: n_rows rows written over n_words distinct (ctx, word) pairs in n_contexts contexts, into a trace of height
    2^log_n; `defect` 0 none, 1 kind > 3, 2 unaligned word access, 3 two accesses of a word in one cycle with a write, 4 the section
    does not fit; `defect_index` the arrival index of the lowest offending access."""
    _fields_ = [("n_rows", C.c_uint64), ("n_words", C.c_uint64), ("n_contexts", C.c_uint64), ("log_n", C.c_int32), ("defect", C.c_int32),
                ("defect_index", C.c_uint64)]

    def __repr__(self):
        return (f"MemSectionInfo(n_rows={self.n_rows}, n_words={self.n_words}, n_contexts={self.n_contexts}, log_n={self.log_n}, "
                f"defect={self.defect}, defect_index={self.defect_index})")


def _mem_accesses(accesses):
    acc = np.ascontiguousarray(accesses, dtype=MEM_ACCESS_DTYPE).reshape(-1)
    return acc, acc.ctypes.data_as(C.c_void_p) if acc.size else None


def _mem_section_result(lib, ctx, rc, info):
    if rc != 0:
        e = MidenHipError(f"libmidenhip error {rc}: {lib.mh_last_error(ctx.h).decode()}")
        e.info = info
        raise e


def memory_section_tile(lib=None):
    """mh_memory_section_tile: rows of one tile of the word-carry scan."""
    lib = lib or load_library()
    lib.mh_memory_section_tile.restype = C.c_uint32
    lib.mh_memory_section_tile.argtypes = []
    return int(lib.mh_memory_section_tile())


def memory_section(ctx, accesses, log_n=None, want_rows=False):
    """mh_memory_section_build: Memory::fill_trace on the device from an access list in program order (MEM_ACCESS_DTYPE records; within a
    word the clocks must not decrease) -> (Trace [2^log_n, 17], MemSectionInfo, row_of); log_n None: max(6, ceil log2 n).  row_of[i] is
    the section row of access i (uint32 [n]) when want_rows, else None.  A defect of the list raises MidenHipError with `e.info`."""
    acc, ap = _mem_accesses(accesses)
    lib = ctx.lib
    lib.mh_memory_section_build.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.POINTER(C.c_void_p), C.c_void_p, C.POINTER(MemSectionInfo)]
    h, info = C.c_void_p(), MemSectionInfo()
    rows = np.zeros(acc.size, dtype=np.uint32) if want_rows else None
    rp = rows.ctypes.data_as(C.c_void_p) if want_rows and acc.size else None
    rc = lib.mh_memory_section_build(ctx.h, ap, acc.size, -1 if log_n is None else int(log_n), C.byref(h), rp, C.byref(info))
    _mem_section_result(lib, ctx, rc, info)
    return Trace.from_handle(ctx, h, int(info.log_n), 17), info, rows


# ---- the hasher controller's trace section (include/midenhip.h mh_hasher_section_build, mh_miden_hasher_section) ----
HASH_OP_DTYPE = np.dtype([("kind", "<u4"), ("count", "<u4"), ("index", "<u8"), ("payload", "<u8")])  # mh_hash_op
HASH_RESULT_DTYPE = np.dtype([("addr", "<u8"), ("state", "<u8", (12,)), ("old_root", "<u8", (4,))])  # mh_hash_result
HASH_PERMUTE, HASH_CONTROL_BLOCK, HASH_BASIC_BLOCK, HASH_MERKLE_VERIFY, HASH_MERKLE_UPDATE = range(5)  # mh_hash_op.kind


class HasherSectionInfo(C.Structure):
    """mh_hasher_section_info: n_rows controller rows (padding included) for n_permutations permutations with n_requests distinct
    pre-states, the final mrupdate_id, into a trace of height 2^log_n; `defect` 0 none, 1 kind > 4, 2 count out of range, 3 invalid
    Merkle index, 4 operands outside the felts, 5 the section does not fit; `defect_index` the lowest offending op."""
    _fields_ = [("n_rows", C.c_uint64), ("n_permutations", C.c_uint64), ("n_requests", C.c_uint64), ("mrupdate_id", C.c_uint64),
                ("log_n", C.c_int32), ("defect", C.c_int32), ("defect_index", C.c_uint64)]

    def __repr__(self):
        return (f"HasherSectionInfo(n_rows={self.n_rows}, n_permutations={self.n_permutations}, n_requests={self.n_requests}, "
                f"mrupdate_id={self.mrupdate_id}, log_n={self.log_n}, defect={self.defect}, defect_index={self.defect_index})")


def _hash_ops(ops, felts):
    o = np.ascontiguousarray(ops, dtype=HASH_OP_DTYPE).reshape(-1)
    f = np.ascontiguousarray(felts, dtype=np.uint64).reshape(-1)
    return o, o.ctypes.data_as(C.c_void_p) if o.size else None, f, f.ctypes.data_as(C.c_void_p) if f.size else None


def hasher_section_tile(lib=None):
    """mh_hasher_section_tile: ops (and permutations) of one tile of the stage's scans."""
    lib = lib or load_library()
    lib.mh_hasher_section_tile.restype = C.c_uint32
    lib.mh_hasher_section_tile.argtypes = []
    return int(lib.mh_hasher_section_tile())


def hasher_section(ctx, ops, felts, log_n=None, want_results=False):
    """mh_hasher_section_build: the hasher controller's rows on the device from the hash operations in program order (HASH_OP_DTYPE
    records whose `payload` points into `felts`, any uint64) -> (Trace [2^log_n, 20], HasherSectionInfo, results); log_n None:
    max(6, ceil log2 n_rows).  results is a HASH_RESULT_DTYPE array (addr, last post-state, old root) when want_results, else None.
    A defect of the list raises MidenHipError with `e.info`."""
    o, op, f, fp = _hash_ops(ops, felts)
    lib = ctx.lib
    lib.mh_hasher_section_build.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_int, C.POINTER(C.c_void_p),
                                            C.c_void_p, C.POINTER(HasherSectionInfo)]
    h, info = C.c_void_p(), HasherSectionInfo()
    res = np.zeros(o.size, dtype=HASH_RESULT_DTYPE) if want_results else None
    rp = res.ctypes.data_as(C.c_void_p) if want_results and o.size else None
    rc = lib.mh_hasher_section_build(ctx.h, op, o.size, fp, f.size, -1 if log_n is None else int(log_n), C.byref(h), rp, C.byref(info))
    _mem_section_result(lib, ctx, rc, info)
    return Trace.from_handle(ctx, h, int(info.log_n), 20), info, res


# ---- the bitwise, ACE and kernel-ROM sections and the whole chiplets trace (include/midenhip.h mh_bitwise_section_build ..
# mh_miden_chiplets_build) ----
BITWISE_OP_DTYPE = np.dtype([("op", "<u4"), ("a", "<u4"), ("b", "<u4")])  # mh_bitwise_op
ACE_EVAL_DTYPE = np.dtype([("ctx", "<u4"), ("ptr", "<u4"), ("clk", "<u4"), ("num_vars", "<u4"), ("num_eval", "<u4"), ("reserved", "<u4"),
                           ("payload", "<u8")])  # mh_ace_eval
BITWISE_AND, BITWISE_XOR = 0, 1  # mh_bitwise_op.op


class BitwiseSectionInfo(C.Structure):
    """mh_bitwise_section_info: n_rows = 8 n_ops rows into a trace of height 2^log_n; `defect` 0 none, 1 op > 1, 2 the section does not
    fit; `defect_index` the lowest offending op."""
    _fields_ = [("n_rows", C.c_uint64), ("log_n", C.c_int32), ("defect", C.c_int32), ("defect_index", C.c_uint64)]

    def __repr__(self):
        return f"BitwiseSectionInfo(n_rows={self.n_rows}, log_n={self.log_n}, defect={self.defect}, defect_index={self.defect_index})"


class AceSectionInfo(C.Structure):
    """mh_ace_section_info: n_rows READ and EVAL rows over n_wires wires and n_gates gates, evaluated in n_rounds rounds; `defect` 0
    none, 1 bad num_vars / num_eval, 2 clk not above the previous evaluation's, 3 operands outside the felts or the address space, 4 a
    bad gate (`defect_gate`), 5 the section does not fit, 6 the circuit does not evaluate to zero; `defect_index` the evaluation."""
    _fields_ = [("n_rows", C.c_uint64), ("n_wires", C.c_uint64), ("n_gates", C.c_uint64), ("n_rounds", C.c_uint64), ("log_n", C.c_int32),
                ("defect", C.c_int32), ("defect_index", C.c_uint64), ("defect_gate", C.c_uint64)]

    def __repr__(self):
        return (f"AceSectionInfo(n_rows={self.n_rows}, n_wires={self.n_wires}, n_gates={self.n_gates}, n_rounds={self.n_rounds}, "
                f"log_n={self.log_n}, defect={self.defect}, defect_index={self.defect_index}, defect_gate={self.defect_gate})")


class KernelRomSectionInfo(C.Structure):
    """mh_kernel_rom_section_info: n_rows distinct declared digests, n_calls calls; `defect` 0 none, 1 a call of an undeclared digest,
    2 the section does not fit; `defect_index` the lowest offending call (1) or the first row without room (2)."""
    _fields_ = [("n_rows", C.c_uint64), ("n_calls", C.c_uint64), ("log_n", C.c_int32), ("defect", C.c_int32), ("defect_index", C.c_uint64)]

    def __repr__(self):
        return (f"KernelRomSectionInfo(n_rows={self.n_rows}, n_calls={self.n_calls}, log_n={self.log_n}, defect={self.defect}, "
                f"defect_index={self.defect_index})")


class ChipletsLists(C.Structure):
    """mh_chiplets_lists: the five lists of one executed program (host pointers and counts)."""
    _fields_ = [("hash_ops", C.c_void_p), ("n_hash_ops", C.c_size_t), ("hash_felts", C.c_void_p), ("n_hash_felts", C.c_size_t),
                ("bitwise_ops", C.c_void_p), ("n_bitwise_ops", C.c_size_t), ("mem_accesses", C.c_void_p), ("n_mem_accesses", C.c_size_t),
                ("ace_evals", C.c_void_p), ("n_ace_evals", C.c_size_t), ("ace_felts", C.c_void_p), ("n_ace_felts", C.c_size_t),
                ("kernel_procs", C.c_void_p), ("n_kernel_procs", C.c_size_t), ("kernel_calls", C.c_void_p), ("n_kernel_calls", C.c_size_t)]


class ChipletsInfo(C.Structure):
    """mh_chiplets_info: the section starts (hasher, bitwise, memory, ACE, kernel ROM), padding_start, trace_len = padding_start + 1,
    log_n; `defect_section` -1 none, 0..4 the first defective section in trace order, 5 the frame (trace_len > 2^log_n), with that
    section's `defect` and `defect_index`; then the five builders' infos."""
    _fields_ = [("start", C.c_uint64 * 5), ("padding_start", C.c_uint64), ("trace_len", C.c_uint64), ("log_n", C.c_int32),
                ("defect_section", C.c_int32), ("defect", C.c_int32), ("reserved", C.c_int32), ("defect_index", C.c_uint64),
                ("hasher", HasherSectionInfo), ("bitwise", BitwiseSectionInfo), ("memory", MemSectionInfo), ("ace", AceSectionInfo),
                ("kernel_rom", KernelRomSectionInfo)]

    def __repr__(self):
        return (f"ChipletsInfo(start={list(self.start)}, padding_start={self.padding_start}, trace_len={self.trace_len}, log_n={self.log_n}, "
                f"defect_section={self.defect_section}, defect={self.defect}, defect_index={self.defect_index})")


def _records(x, dtype):
    """a contiguous 1-d array of `dtype` records; an empty sequence is an empty list"""
    return np.ascontiguousarray(x, dtype=dtype).reshape(-1) if len(x) else np.zeros(0, dtype=dtype)


def _bitwise_ops(ops):
    o = _records(ops, BITWISE_OP_DTYPE)
    return o, o.ctypes.data_as(C.c_void_p) if o.size else None


def _ace_evals(evals, felts):
    e = _records(evals, ACE_EVAL_DTYPE)
    f = np.ascontiguousarray(felts, dtype=np.uint64).reshape(-1)
    return e, e.ctypes.data_as(C.c_void_p) if e.size else None, f, f.ctypes.data_as(C.c_void_p) if f.size else None


def _digests(d):
    a = np.ascontiguousarray(d, dtype=np.uint64).reshape(-1, 4)
    return a, a.ctypes.data_as(C.c_void_p) if a.size else None


def ace_section_tile(lib=None):
    """mh_ace_section_tile: evaluations of one tile of the plan's scan."""
    lib = lib or load_library()
    lib.mh_ace_section_tile.restype = C.c_uint32
    lib.mh_ace_section_tile.argtypes = []
    return int(lib.mh_ace_section_tile())


def bitwise_section(ctx, ops, log_n=None, want_results=False):
    """mh_bitwise_section_build: the bitwise chiplet's rows on the device from the operations in program order (BITWISE_OP_DTYPE
    records) -> (Trace [2^log_n, 13], BitwiseSectionInfo, results); log_n None: max(6, ceil log2 n_rows).  results is the uint32 result
    per op when want_results, else None.  A defect of the list raises MidenHipError with `e.info`."""
    o, op = _bitwise_ops(ops)
    lib = ctx.lib
    lib.mh_bitwise_section_build.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.POINTER(C.c_void_p), C.c_void_p,
                                             C.POINTER(BitwiseSectionInfo)]
    h, info = C.c_void_p(), BitwiseSectionInfo()
    res = np.zeros(o.size, dtype=np.uint32) if want_results else None
    rp = res.ctypes.data_as(C.c_void_p) if want_results and o.size else None
    rc = lib.mh_bitwise_section_build(ctx.h, op, o.size, -1 if log_n is None else int(log_n), C.byref(h), rp, C.byref(info))
    _mem_section_result(lib, ctx, rc, info)
    return Trace.from_handle(ctx, h, int(info.log_n), 13), info, res


def ace_section(ctx, evals, felts, log_n=None):
    """mh_ace_section_build: the ACE chiplet's rows on the device from the circuit evaluations in clock order (ACE_EVAL_DTYPE records
    whose `payload` points into `felts`: 2 num_vars felts as read from memory, then num_eval instructions) -> (Trace [2^log_n, 16],
    AceSectionInfo); log_n None: max(6, ceil log2 n_rows).  A defect of the list raises MidenHipError with `e.info`."""
    e, ep, f, fp = _ace_evals(evals, felts)
    lib = ctx.lib
    lib.mh_ace_section_build.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_int, C.POINTER(C.c_void_p),
                                         C.POINTER(AceSectionInfo)]
    h, info = C.c_void_p(), AceSectionInfo()
    rc = lib.mh_ace_section_build(ctx.h, ep, e.size, fp, f.size, -1 if log_n is None else int(log_n), C.byref(h), C.byref(info))
    _mem_section_result(lib, ctx, rc, info)
    return Trace.from_handle(ctx, h, int(info.log_n), 16), info


def kernel_rom_section(ctx, procs, calls, log_n=None, want_digests=False):
    """mh_kernel_rom_section_build: the kernel ROM's rows on the device from the declared procedure digests and the called digests
    (uint64 [n][4] each) -> (Trace [2^log_n, 5], KernelRomSectionInfo, digests); log_n None: max(6, ceil log2 n_rows).  digests is the
    uint64 [n_rows, 4] array of the rows' digests in trace order when want_digests, else None.  A defect raises MidenHipError with
    `e.info`."""
    p, pp = _digests(procs)
    k, kp = _digests(calls)
    lib = ctx.lib
    lib.mh_kernel_rom_section_build.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_int, C.POINTER(C.c_void_p),
                                                C.c_void_p, C.POINTER(KernelRomSectionInfo)]
    h, info = C.c_void_p(), KernelRomSectionInfo()
    dig = np.zeros((p.shape[0], 4), dtype=np.uint64) if want_digests else None
    dp = dig.ctypes.data_as(C.c_void_p) if want_digests and dig.size else None
    rc = lib.mh_kernel_rom_section_build(ctx.h, pp, p.shape[0], kp, k.shape[0], -1 if log_n is None else int(log_n), C.byref(h), dp, C.byref(info))
    _mem_section_result(lib, ctx, rc, info)
    return Trace.from_handle(ctx, h, int(info.log_n), 5), info, (dig[:int(info.n_rows)] if want_digests else None)


# ---- the precompile prover's Keccak round and sponge traces (include/midenhip.h mh_keccak_round_program .. mh_keccak_traces_build) ----
KECCAK_MSG_DTYPE = np.dtype([("offset", "<u8"), ("len", "<u8"), ("chunk_head", "<u8")])  # mh_keccak_msg


class KeccakTracesInfo(C.Structure):
    """mh_keccak_traces_info: n_perms blocks = permutations, sponge_rows = 32 n_perms active sponge rows, the least heights of the two
    traces; `defect_kind` 0 none, 1 offset + len past the bytes, 2 4 chunk_head + lanes not below 2^32, 3 more than 2^24 rows, 4 a NULL
    pointer, 5 / 6 log_round / log_sponge below the height needed (`defect_index` = the rows needed); else `defect_index` the message."""
    _fields_ = [("n_perms", C.c_uint64), ("sponge_rows", C.c_uint64), ("round_rows_needed", C.c_uint64), ("sponge_rows_needed", C.c_uint64),
                ("defect_kind", C.c_int32), ("defect_index", C.c_uint64)]

    def __repr__(self):
        return (f"KeccakTracesInfo(n_perms={self.n_perms}, sponge_rows={self.sponge_rows}, round_rows_needed={self.round_rows_needed}, "
                f"sponge_rows_needed={self.sponge_rows_needed}, defect_kind={self.defect_kind}, defect_index={self.defect_index})")


def keccak_round_program(lib=None):
    """mh_keccak_round_program (host only): the library's round programme -> [(op, shift, back_a, back_b, dst_mult)] * 128."""
    lib = lib or load_library()
    out = np.zeros((128, 5), dtype=np.int32)
    lib.mh_keccak_round_program.argtypes = [C.c_void_p]
    if lib.mh_keccak_round_program(out.ctypes.data_as(C.c_void_p)) != 0:
        raise MidenHipError("mh_keccak_round_program failed")
    return [tuple(int(x) for x in row) for row in out]


def keccak_round_levels(lib=None):
    """mh_keccak_round_levels (host only): the level of each of the 128 slots in the device schedule, -1 for a NOP slot."""
    lib = lib or load_library()
    out = np.zeros(128, dtype=np.int32)
    lib.mh_keccak_round_levels.argtypes = [C.c_void_p]
    if lib.mh_keccak_round_levels(out.ctypes.data_as(C.c_void_p)) != 0:
        raise MidenHipError("mh_keccak_round_levels failed")
    return [int(x) for x in out]


def keccak_round_trace(ctx, states, log_n=None, want_outputs=False):
    """mh_keccak_round_trace_build: KeccakRoundAir's main trace on the device from the permutations' 25-lane inputs (uint64 [n, 25])
    -> Trace [2^log_n, 68], or (Trace, outputs uint64 [n, 25] = Keccak-f[1600] of each state) when want_outputs.  log_n None: the
    least, max(2, next_pow2(ceil(max(n, 1) / 2) * 3200)); a smaller one raises MidenHipError with the rows needed."""
    s = np.ascontiguousarray(states, dtype=np.uint64).reshape(-1, 25)
    n = s.shape[0]
    lib = ctx.lib
    lib.mh_keccak_round_trace_build.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.POINTER(C.c_void_p), C.c_void_p]
    h = C.c_void_p()
    outs = np.zeros((n, 25), dtype=np.uint64) if want_outputs else None
    op = outs.ctypes.data_as(C.c_void_p) if want_outputs and n else None
    least = max(1, (-(-max(n, 1) // 2) * 3200 - 1).bit_length())
    ctx.check(lib.mh_keccak_round_trace_build(ctx.h, s.ctypes.data_as(C.c_void_p) if n else None, n, -1 if log_n is None else int(log_n),
                                              C.byref(h), op))
    t = Trace.from_handle(ctx, h, least if log_n is None else int(log_n), 68)
    return (t, outs) if want_outputs else t


def keccak_traces(ctx, messages, chunk_heads, log_round=None, log_sponge=None, want_digests=False):
    """mh_keccak_traces_build: the main traces of KeccakRoundAir and KeccakSpongeAir on the device from the messages a session hashes
    (bytes-like each) and their chunk-tape bases in chunks (ChunkRequires.require's chunk_head) -> (round Trace [2^log_round, 68],
    sponge Trace [2^log_sponge, 67], KeccakTracesInfo[, digests uint8 [n, 32]]).  log_* None: the least heights.  A refusal raises
    MidenHipError with `e.info`."""
    msgs = [bytes(m) for m in messages]
    if len(msgs) != len(chunk_heads):
        raise MidenHipError("keccak_traces: one chunk head per message expected")
    rec = np.zeros(len(msgs), dtype=KECCAK_MSG_DTYPE)
    at = 0
    for i, (m, head) in enumerate(zip(msgs, chunk_heads)):
        rec[i] = (at, len(m), int(head))
        at += len(m)
    data = np.frombuffer(b"".join(msgs), dtype=np.uint8)
    return keccak_traces_raw(ctx, data, rec, log_round, log_sponge, want_digests)


def keccak_traces_raw(ctx, data, msgs, log_round=None, log_sponge=None, want_digests=False):
    """keccak_traces on the ABI's own arguments: `data` uint8, `msgs` KECCAK_MSG_DTYPE records (offset, len, chunk_head) into it."""
    data = np.ascontiguousarray(data, dtype=np.uint8).reshape(-1)
    rec = _records(msgs, KECCAK_MSG_DTYPE)
    lib = ctx.lib
    lib.mh_keccak_traces_build.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_int, C.c_int, C.POINTER(C.c_void_p),
                                           C.POINTER(C.c_void_p), C.c_void_p, C.POINTER(KeccakTracesInfo)]
    hr, hs, info = C.c_void_p(), C.c_void_p(), KeccakTracesInfo()
    dig = np.zeros((rec.size, 32), dtype=np.uint8) if want_digests else None
    dp = dig.ctypes.data_as(C.c_void_p) if want_digests and rec.size else None
    rc = lib.mh_keccak_traces_build(ctx.h, data.ctypes.data_as(C.c_void_p) if data.size else None, data.size,
                                    rec.ctypes.data_as(C.c_void_p) if rec.size else None, rec.size, -1 if log_round is None else int(log_round),
                                    -1 if log_sponge is None else int(log_sponge), C.byref(hr), C.byref(hs), dp, C.byref(info))
    _mem_section_result(lib, ctx, rc, info)
    lr = int(info.round_rows_needed).bit_length() - 1 if log_round is None else int(log_round)
    ls = int(info.sponge_rows_needed).bit_length() - 1 if log_sponge is None else int(log_sponge)
    out = (Trace.from_handle(ctx, hr, lr, 68), Trace.from_handle(ctx, hs, ls, 67), info)
    return out + (dig,) if want_digests else out


# ---- the precompile prover's Poseidon2 chiplet trace (include/midenhip.h mh_poseidon2_chiplet_plan, mh_poseidon2_chiplet_trace_build) ----
P2C_ABSORPTION_DTYPE = np.dtype([("cap", "<u8", (4,)), ("n_blocks", "<u8"), ("in_mult", "<u8"), ("out_mult", "<u8")])  # mh_p2c_absorption


class Poseidon2ChipletInfo(C.Structure):
    """mh_p2c_info: the ledger's absorptions, cycles and levels, the least height and the height taken; `defect_kind` 0 none, 1 a NULL
    pointer, 2 n_blocks = 0 (`defect_index` the absorption), 3 the n_blocks do not add up to n_cycles (the first absorption that runs
    past, n_abs when the list ends short), 4 a bad reference (2 cycle + half), 5 more than 2^20 cycles, 6 log_n below the height needed
    (the rows needed)."""
    _fields_ = [("n_absorptions", C.c_uint64), ("n_cycles", C.c_uint64), ("n_levels", C.c_uint64), ("rows_needed", C.c_uint64),
                ("log_n", C.c_int32), ("defect_kind", C.c_int32), ("defect_index", C.c_uint64)]

    def __repr__(self):
        return (f"Poseidon2ChipletInfo(n_absorptions={self.n_absorptions}, n_cycles={self.n_cycles}, n_levels={self.n_levels}, "
                f"rows_needed={self.rows_needed}, log_n={self.log_n}, defect_kind={self.defect_kind}, defect_index={self.defect_index})")


def _p2c_args(absorptions, blocks, refs):
    a = _records(absorptions, P2C_ABSORPTION_DTYPE)
    b = np.ascontiguousarray(blocks, dtype=np.uint64).reshape(-1, 8)
    r = None if refs is None else np.ascontiguousarray(refs, dtype=np.int64).reshape(-1, 2)
    if r is not None and r.shape[0] != b.shape[0]:
        raise MidenHipError("poseidon2_chiplet: one pair of references per block expected")
    return a, b, r


def poseidon2_chiplet_plan(absorptions, n_cycles, refs=None, lib=None):
    """mh_poseidon2_chiplet_plan (host only): validates the ledger -> (start uint64 [n_abs], level uint32 [n_abs], Poseidon2ChipletInfo).
    `absorptions`: P2C_ABSORPTION_DTYPE records, `refs` int64 [n_cycles, 2] or None.  A defect raises MidenHipError with `e.info`."""
    lib = lib or load_library()
    a = _records(absorptions, P2C_ABSORPTION_DTYPE)
    r = None if refs is None else np.ascontiguousarray(refs, dtype=np.int64).reshape(-1, 2)
    if r is not None and r.shape[0] != int(n_cycles):
        raise MidenHipError("poseidon2_chiplet_plan: one pair of references per cycle expected")
    start, level, info = np.zeros(a.size, dtype=np.uint64), np.zeros(a.size, dtype=np.uint32), Poseidon2ChipletInfo()
    lib.mh_poseidon2_chiplet_plan.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.POINTER(Poseidon2ChipletInfo)]
    rc = lib.mh_poseidon2_chiplet_plan(a.ctypes.data_as(C.c_void_p) if a.size else None, a.size, r.ctypes.data_as(C.c_void_p) if r is not None and r.size else None,
                                       int(n_cycles), start.ctypes.data_as(C.c_void_p) if a.size else None,
                                       level.ctypes.data_as(C.c_void_p) if a.size else None, C.byref(info))
    if rc != 0:
        e = MidenHipError(f"mh_poseidon2_chiplet_plan: defect {info.defect_kind}, index {info.defect_index}")
        e.info = info
        raise e
    return start, level, info


def poseidon2_chiplet_trace(ctx, absorptions, blocks, refs=None, log_n=None, want_digests=False, want_outputs=False):
    """mh_poseidon2_chiplet_trace_build: Poseidon2Air's main trace on the device from the absorption ledger -- `absorptions`
    P2C_ABSORPTION_DTYPE records (cap, n_blocks, in_mult, out_mult), `blocks` uint64 [n_cycles, 8] in absorption order, `refs` int64
    [n_cycles, 2] (-1: the literal half; else the earlier absorption whose digest is that half) or None -> (Trace [2^log_n, 32],
    Poseidon2ChipletInfo[, digests uint64 [n_abs, 4]][, outputs uint64 [n_cycles, 12]]).  log_n None: the least height,
    max(16, next_pow2(16 n_cycles)).  A refusal raises MidenHipError with `e.info`."""
    a, b, r = _p2c_args(absorptions, blocks, refs)
    lib = ctx.lib
    lib.mh_poseidon2_chiplet_trace_build.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.POINTER(C.c_void_p),
                                                     C.c_void_p, C.c_void_p, C.POINTER(Poseidon2ChipletInfo)]
    h, info = C.c_void_p(), Poseidon2ChipletInfo()
    dig = np.zeros((a.size, 4), dtype=np.uint64) if want_digests else None
    outs = np.zeros((b.shape[0], 12), dtype=np.uint64) if want_outputs else None
    rc = lib.mh_poseidon2_chiplet_trace_build(ctx.h, a.ctypes.data_as(C.c_void_p) if a.size else None, a.size, b.ctypes.data_as(C.c_void_p) if b.size else None,
                                              r.ctypes.data_as(C.c_void_p) if r is not None and r.size else None, b.shape[0],
                                              -1 if log_n is None else int(log_n), C.byref(h), dig.ctypes.data_as(C.c_void_p) if want_digests and a.size else None,
                                              outs.ctypes.data_as(C.c_void_p) if want_outputs and b.size else None, C.byref(info))
    _mem_section_result(lib, ctx, rc, info)
    out = (Trace.from_handle(ctx, h, int(info.log_n), 32), info)
    return out + ((dig,) if want_digests else ()) + ((outs,) if want_outputs else ())


# ---- the precompile prover's UintStoreMul and UintAdd traces (include/midenhip.h mh_uint_traces_plan, mh_uint_traces_build) ----
UINT_ROW_DTYPE = np.dtype([("ptr", "<u4"), ("bound_ptr", "<u4"), ("value", "<u4", (8,)), ("val_reads", "<u4"), ("limb_reads", "<u4")])  # mh_uint_row
UINT_MUL_OP_DTYPE = np.dtype([("a", "<u4"), ("b", "<u4"), ("c", "<u4"), ("r", "<u4"), ("bound", "<u4"), ("kappa_a", "<u4"), ("kappa_c", "<u4"),
                              ("is_sub", "<u4"), ("mult", "<u8")])                                                                     # mh_uint_mul_op
UINT_ADD_OP_DTYPE = np.dtype([("a", "<u4"), ("b", "<u4"), ("c", "<u4"), ("bound", "<u4"), ("nz", "<u4"), ("reserved", "<u4"), ("mult", "<u8")])  # mh_uint_add_op


class UintTracesInfo(C.Structure):
    """mh_uint_traces_info: the lists' sizes, the least heights of the two traces and the ones taken; `defect_section` 0 store, 1 multiply,
    2 add; `defect_kind` 0 none, 1..7 the planner's (a NULL pointer; too many rows or padding pointers past 2^32; log below the height,
    index the rows needed; ptr 0 or not ascending; a gap >= 2^16; bound_ptr not stored; value above its bound), 8..14 the device's (a
    pointer not stored, operand named; kappa >= 2^16; r not the canonical remainder / the addition holds for no k; quotient >= 2^272;
    underflow beyond two moduli; a carry outside its window; nz with b = 0)."""
    _fields_ = [("n_store", C.c_uint64), ("n_mul", C.c_uint64), ("n_add", C.c_uint64), ("usm_rows_needed", C.c_uint64), ("usm_rows", C.c_uint64),
                ("add_rows_needed", C.c_uint64), ("add_rows", C.c_uint64), ("defect_section", C.c_int32), ("defect_kind", C.c_int32),
                ("defect_index", C.c_uint64), ("defect_operand", C.c_int32), ("reserved", C.c_int32)]

    def __repr__(self):
        return (f"UintTracesInfo(n_store={self.n_store}, n_mul={self.n_mul}, n_add={self.n_add}, usm_rows_needed={self.usm_rows_needed}, "
                f"usm_rows={self.usm_rows}, add_rows_needed={self.add_rows_needed}, add_rows={self.add_rows}, defect_section={self.defect_section}, "
                f"defect_kind={self.defect_kind}, defect_index={self.defect_index}, defect_operand={self.defect_operand})")


def _uint_lists(rows, muls, adds, sort=True):
    """the three record arrays, the store sorted by ptr (the order of the trace; the device does not sort)"""
    r, m, a = _records(rows, UINT_ROW_DTYPE), _records(muls, UINT_MUL_OP_DTYPE), _records(adds, UINT_ADD_OP_DTYPE)
    if sort and r.size > 1 and not (r["ptr"][1:] >= r["ptr"][:-1]).all():
        r = np.ascontiguousarray(r[np.argsort(r["ptr"], kind="stable")])
    return r, m, a


def _void_p(x):
    return x.ctypes.data_as(C.c_void_p) if x.size else None


def uint_traces_plan(rows, muls, adds, log_usm=None, log_add=None, lib=None, sort=True):
    """mh_uint_traces_plan (host only): validates the store and gives the heights -> (bound_index uint32 [n_store], UintTracesInfo).
    `rows` UINT_ROW_DTYPE, `muls` UINT_MUL_OP_DTYPE, `adds` UINT_ADD_OP_DTYPE records.  A defect raises MidenHipError with `e.info`."""
    lib = lib or load_library()
    r, m, a = _uint_lists(rows, muls, adds, sort)
    bound_index, info = np.zeros(r.size, dtype=np.uint32), UintTracesInfo()
    lib.mh_uint_traces_plan.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_int, C.c_int, C.c_void_p,
                                        C.POINTER(UintTracesInfo)]
    rc = lib.mh_uint_traces_plan(_void_p(r), r.size, _void_p(m), m.size, _void_p(a), a.size, -1 if log_usm is None else int(log_usm),
                                 -1 if log_add is None else int(log_add), _void_p(bound_index), C.byref(info))
    if rc != 0:
        e = MidenHipError(f"mh_uint_traces_plan: section {info.defect_section}, defect {info.defect_kind}, index {info.defect_index}")
        e.info = info
        raise e
    return bound_index, info


def uint_traces(ctx, rows, muls, adds, log_usm=None, log_add=None, sort=True):
    """mh_uint_traces_build: UintStoreMulAir's and UintAddAir's main traces on the device from the ledgers -- `rows` UINT_ROW_DTYPE records
    (ptr, bound_ptr, value in eight 32-bit limbs, the reads from outside the two chiplets; sorted by ptr here), `muls` UINT_MUL_OP_DTYPE
    (kappa_a a b +- kappa_c c = r mod bound + 1 over pointers, mult), `adds` UINT_ADD_OP_DTYPE (a + b = c mod bound + 1, pointer 0 in b / c:
    absent) -> (Trace [usm_rows, 44], Trace [add_rows, 30], UintTracesInfo).  log_* None: the least heights.  sort=False hands the store
    over as it is.  A refusal raises MidenHipError with `e.info` (section, kind, index, operand)."""
    r, m, a = _uint_lists(rows, muls, adds, sort)
    lib = ctx.lib
    lib.mh_uint_traces_build.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_int, C.c_int,
                                         C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(UintTracesInfo)]
    hu, ha, info = C.c_void_p(), C.c_void_p(), UintTracesInfo()
    rc = lib.mh_uint_traces_build(ctx.h, _void_p(r), r.size, _void_p(m), m.size, _void_p(a), a.size, -1 if log_usm is None else int(log_usm),
                                  -1 if log_add is None else int(log_add), C.byref(hu), C.byref(ha), C.byref(info))
    _mem_section_result(lib, ctx, rc, info)
    return (Trace.from_handle(ctx, hu, int(info.usm_rows).bit_length() - 1, 44), Trace.from_handle(ctx, ha, int(info.add_rows).bit_length() - 1, 30), info)


# ---- the precompile prover's EcGroups, EcPointStore, EcGroupAdd and EcMsm traces (include/midenhip.h mh_ec_traces_plan, mh_ec_traces_build) ----
EC_GROUP_DTYPE = np.dtype([("a_ptr", "<u4"), ("b_ptr", "<u4"), ("bound_ptr", "<u4"), ("sbound_ptr", "<u4"), ("ext_reads", "<u8")])             # mh_ec_group
EC_POINT_DTYPE = np.dtype([("group", "<u4"), ("x_ptr", "<u4"), ("y_ptr", "<u4"), ("u_ptr", "<u4"), ("w_ptr", "<u4"), ("kind", "<u4"),
                           ("ext_reads", "<u8")])                                                                                              # mh_ec_point
EC_ADD_OP_DTYPE = np.dtype([("group", "<u4"), ("p", "<u4"), ("q", "<u4"), ("r", "<u4"), ("kind", "<u4"), ("mints", "<u4"), ("t", "<u4", (6,)),
                            ("mult", "<u8")])                                                                                                  # mh_ec_add_op
MSM_EXPR_DTYPE = np.dtype([("kind", "<u4"), ("group", "<u4"), ("val", "<u4"), ("a_expr", "<u4"), ("b_expr", "<u4"), ("n_rows", "<u4"),
                           ("neg_minted", "<u4"), ("reserved", "<u4"), ("ext_mult", "<u8"), ("claim_mult", "<u8")])                            # mh_msm_expr
MSM_TERM_DTYPE = np.dtype([("base", "<u4"), ("scalar", "<u4")])                                                                                # mh_msm_term


class EcTracesInfo(C.Structure):
    """mh_ec_traces_info: the lists' sizes, the least heights of the four traces and the ones taken; `defect_section` 0 groups, 1 points,
    2 add, 3 msm; `defect_kind` 0 none, 1..7 the planner's (a NULL list; too many rows or a log above 24; log below the height, index the
    rows needed; a point's group out of range; a point kind or its pointers; an expression's kind or n_rows; an operand that is not an
    earlier expression), 8..15 the device's (a pointer out of range, operand named; an addition's kind or mints; another group; the kind
    against the points at infinity; a mint's ordering; bases not ascending; a merge or neg that does not follow its operands; an intro
    whose val is not its base)."""
    _fields_ = [("n_groups", C.c_uint64), ("n_points", C.c_uint64), ("n_add", C.c_uint64), ("n_exprs", C.c_uint64), ("n_terms", C.c_uint64),
                ("groups_rows_needed", C.c_uint64), ("groups_rows", C.c_uint64), ("points_rows_needed", C.c_uint64), ("points_rows", C.c_uint64),
                ("add_rows_needed", C.c_uint64), ("add_rows", C.c_uint64), ("msm_rows_needed", C.c_uint64), ("msm_rows", C.c_uint64),
                ("defect_section", C.c_int32), ("defect_kind", C.c_int32), ("defect_index", C.c_uint64), ("defect_operand", C.c_int32),
                ("reserved", C.c_int32)]

    def __repr__(self):
        return "EcTracesInfo(" + ", ".join(f"{n}={getattr(self, n)}" for n, _ in self._fields_ if n != "reserved") + ")"


_EC_LIST_DTYPES = (EC_GROUP_DTYPE, EC_POINT_DTYPE, EC_ADD_OP_DTYPE, MSM_EXPR_DTYPE, MSM_TERM_DTYPE)


def _ec_call_args(lists, logs):
    """the five record arrays, and the ABI's arguments for them and the four logs"""
    recs = [_records(x, dt) for x, dt in zip(lists, _EC_LIST_DTYPES)]
    args = [v for r in recs for v in (_void_p(r), r.size)] + [-1 if l is None else int(l) for l in logs]
    return recs, args


def ec_traces_plan(groups, points, adds, exprs, terms, log_groups=-1, log_points=-1, log_add=-1, log_msm=-1, lib=None):
    """mh_ec_traces_plan (host only): validates what one record shows and gives the heights -> (row_start uint32 [n_exprs], EcTracesInfo).
    EC_GROUP_DTYPE, EC_POINT_DTYPE, EC_ADD_OP_DTYPE, MSM_EXPR_DTYPE, MSM_TERM_DTYPE records.  A defect raises MidenHipError with `e.info`."""
    lib = lib or load_library()
    recs, args = _ec_call_args((groups, points, adds, exprs, terms), (log_groups, log_points, log_add, log_msm))
    row_start, info = np.zeros(recs[3].size, dtype=np.uint32), EcTracesInfo()
    lib.mh_ec_traces_plan.argtypes = [C.c_void_p, C.c_size_t] * 5 + [C.c_int] * 4 + [C.c_void_p, C.POINTER(EcTracesInfo)]
    rc = lib.mh_ec_traces_plan(*args, _void_p(row_start), C.byref(info))
    if rc != 0:
        e = MidenHipError(f"mh_ec_traces_plan: section {info.defect_section}, defect {info.defect_kind}, index {info.defect_index}, "
                          f"operand {info.defect_operand}")
        e.info = info
        raise e
    return row_start, info


def ec_traces(ctx, groups, points, adds, exprs, terms, log_groups=-1, log_points=-1, log_add=-1, log_msm=-1):
    """mh_ec_traces_build: EcGroupsAir's, EcPointStoreAir's, EcGroupAddAir's and EcMsmAir's main traces on the device from the ledgers --
    `groups` EC_GROUP_DTYPE (row i is group i + 1), `points` EC_POINT_DTYPE (row i is point i + 1; kind 0 member, 1 point at infinity,
    2 closure-certified), `adds` EC_ADD_OP_DTYPE (kind 0 pai_p .. 5 generic), `exprs` MSM_EXPR_DTYPE (kind 0 intro, 1 combine, 2 neg) and
    `terms` MSM_TERM_DTYPE (the expressions' rows, concatenated) -> ((Trace [., 6], Trace [., 14], Trace [., 21], Trace [., 38]),
    EcTracesInfo).  ext_reads / ext_mult are the reads from outside the four chiplets; the device adds the rest.  log_* -1 (or None): the
    least heights.  A refusal raises MidenHipError with `e.info` (section, kind, index, operand)."""
    recs, args = _ec_call_args((groups, points, adds, exprs, terms), (log_groups, log_points, log_add, log_msm))
    lib = ctx.lib
    lib.mh_ec_traces_build.argtypes = [C.c_void_p] + [C.c_void_p, C.c_size_t] * 5 + [C.c_int] * 4 + [C.POINTER(C.c_void_p)] * 4 + [C.POINTER(EcTracesInfo)]
    hs, info = [C.c_void_p() for _ in range(4)], EcTracesInfo()
    rc = lib.mh_ec_traces_build(ctx.h, *args, *[C.byref(h) for h in hs], C.byref(info))
    _mem_section_result(lib, ctx, rc, info)
    rows = (info.groups_rows, info.points_rows, info.add_rows, info.msm_rows)
    return tuple(Trace.from_handle(ctx, h, int(n).bit_length() - 1, w) for h, n, w in zip(hs, rows, (6, 14, 21, 38))), info


# ---- the precompile prover's ChunkNode and TranscriptEval traces (include/midenhip.h mh_chunk_node_*, mh_transcript_eval_*) ----
KN_RECORD_DTYPE = np.dtype([("offset", "<u8"), ("len", "<u8"), ("chunk_head", "<u8"), ("sponge_head", "<u8"), ("perm_chunks", "<u8"),
                            ("perm_digest_chunks", "<u8"), ("perm_keccak", "<u8"), ("out_mult", "<u8")])                                      # mh_kn_record
TE_NODE_DTYPE = np.dtype([("kind", "<u4"), ("op", "<u4"), ("lhs", "<i8"), ("rhs", "<i8"), ("perm", "<u8"), ("ptr", "<u8"), ("bound_ptr", "<u8"),
                          ("group", "<u8"), ("expr", "<u8")])                                                                                  # mh_te_node
TE_TERM_DTYPE = np.dtype([("base_node", "<u4"), ("scalar_node", "<u4")])                                                                       # mh_te_term
TE_ZERO, TE_AND, TE_UINT_LEAF, TE_UINT_PIN, TE_UINT_OP, TE_EC_CREATE, TE_EC_PAI, TE_EC_OP, TE_EC_MSM = range(9)                                # mh_te_node.kind


class ChunkNodeInfo(C.Structure):
    """mh_chunk_node_info: the records, the chunk rows, the cycles of p2, the least height and the one taken; `defect_kind` 0 none, 1..7 the
    planner's (a NULL pointer or a p2 of another context or width; offset + len past n_bytes; chunk_head not the running sum; sponge_head
    not a multiple of 32; a cycle beyond p2; more than 2^24 rows or a log above 24; log below the height, index the rows needed), 8, 9 the
    device's (a chain that is not one absorption of p2; a digest cycle that does not end one)."""
    _fields_ = [("n_records", C.c_uint64), ("n_chunks", C.c_uint64), ("p2_cycles", C.c_uint64), ("rows_needed", C.c_uint64), ("rows", C.c_uint64),
                ("defect_kind", C.c_int32), ("defect_operand", C.c_int32), ("defect_index", C.c_uint64)]

    def __repr__(self):
        return "ChunkNodeInfo(" + ", ".join(f"{n}={getattr(self, n)}" for n, _ in self._fields_) + ")"


class TranscriptEvalInfo(C.Structure):
    """mh_transcript_eval_info: the lists' sizes, the cycles of p2, the active rows, the ZERO nodes other than the root, the least height
    and the one taken; `defect_kind` 0 none, 1..7 the planner's (a NULL pointer or a p2 of another context or width; an unknown kind or
    op; a source, literal, term span or term node out of range; a root out of range or not truthy; a cycle beyond p2; more than 2^24 rows
    or a log above 24; log below the height, index the rows needed), 8..15 the device's (an operand of the wrong class; different moduli;
    an `is` over distinct pointers; a truthy node not read once or the root read; a value node nobody reads; a perm that is not a
    one-block absorption; an MSM span that is not one absorption; an external cycle that does not end one)."""
    _fields_ = [("n_nodes", C.c_uint64), ("n_terms", C.c_uint64), ("n_lit", C.c_uint64), ("p2_cycles", C.c_uint64), ("active_rows", C.c_uint64),
                ("n_zero", C.c_uint64), ("rows_needed", C.c_uint64), ("rows", C.c_uint64), ("defect_kind", C.c_int32), ("defect_operand", C.c_int32),
                ("defect_index", C.c_uint64)]

    def __repr__(self):
        return "TranscriptEvalInfo(" + ", ".join(f"{n}={getattr(self, n)}" for n, _ in self._fields_) + ")"


def _plan_refused(entry, info):
    e = MidenHipError(f"{entry}: defect {info.defect_kind}, index {info.defect_index}, operand {info.defect_operand}")
    e.info = info
    return e


def _cn_call_args(data, digests, records):
    d = np.ascontiguousarray(np.frombuffer(bytes(data), dtype=np.uint8) if isinstance(data, (bytes, bytearray)) else data, dtype=np.uint8).reshape(-1)
    g = np.ascontiguousarray(digests, dtype=np.uint8).reshape(-1, 32)
    r = _records(records, KN_RECORD_DTYPE)
    if g.shape[0] != r.size:
        raise MidenHipError("chunk_node: one 32-byte digest per record expected")
    return (d, g, r), [_void_p(d), d.size, _void_p(g), _void_p(r), r.size]


def chunk_node_plan(data, digests, records, p2_cycles, log_n=-1, lib=None):
    """mh_chunk_node_plan (host only): validates the records against the bytes and the cycles of the Poseidon2 trace and gives the height
    -> ChunkNodeInfo.  A defect raises MidenHipError with `e.info`."""
    lib = lib or load_library()
    keep, args = _cn_call_args(data, digests, records)
    info = ChunkNodeInfo()
    lib.mh_chunk_node_plan.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_size_t, C.c_uint64, C.c_int, C.POINTER(ChunkNodeInfo)]
    if lib.mh_chunk_node_plan(*args, int(p2_cycles), -1 if log_n is None else int(log_n), C.byref(info)) != 0:
        raise _plan_refused("mh_chunk_node_plan", info)
    return info


def chunk_node_trace(ctx, p2, data, digests, records, log_n=-1):
    """mh_chunk_node_trace_build: ChunkNodeAir's main trace on the device -- `p2` the device-resident Poseidon2 chiplet Trace
    (poseidon2_chiplet_trace on this context), `data` the message bytes, `digests` uint8 [n, 32] (keccak_traces' digests), `records`
    KN_RECORD_DTYPE (offset, len, chunk_head, sponge_head, perm_chunks, perm_digest_chunks, perm_keccak, out_mult), one per distinct
    hashed input -> (Trace [., 42], ChunkNodeInfo).  The three digests of a node row are read from `p2` on the device.  log_n -1 (or
    None): the least height.  A refusal raises MidenHipError with `e.info` (kind, index, operand)."""
    keep, args = _cn_call_args(data, digests, records)
    lib = ctx.lib
    lib.mh_chunk_node_trace_build.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_size_t, C.c_int,
                                              C.POINTER(C.c_void_p), C.POINTER(ChunkNodeInfo)]
    h, info = C.c_void_p(), ChunkNodeInfo()
    rc = lib.mh_chunk_node_trace_build(ctx.h, p2.h, *args, -1 if log_n is None else int(log_n), C.byref(h), C.byref(info))
    _mem_section_result(lib, ctx, rc, info)
    return Trace.from_handle(ctx, h, int(info.rows).bit_length() - 1, 42), info


def _te_call_args(nodes, terms, limbs, root):
    n, t = _records(nodes, TE_NODE_DTYPE), _records(terms, TE_TERM_DTYPE)
    lit = np.ascontiguousarray(limbs, dtype=np.uint32).reshape(-1, 8)
    return (n, t, lit), [_void_p(n), n.size, _void_p(t), t.size, _void_p(lit), lit.shape[0], int(root)]


def transcript_eval_plan(nodes, terms, limbs, root, p2_cycles, log_n=-1, lib=None):
    """mh_transcript_eval_plan (host only): validates kinds, sources and cycles and gives the height and every node's first row
    -> (row_start uint32 [n_nodes], TranscriptEvalInfo).  A defect raises MidenHipError with `e.info`."""
    lib = lib or load_library()
    keep, args = _te_call_args(nodes, terms, limbs, root)
    row_start, info = np.zeros(keep[0].size, dtype=np.uint32), TranscriptEvalInfo()
    lib.mh_transcript_eval_plan.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_uint64, C.c_uint64, C.c_int,
                                            C.c_void_p, C.POINTER(TranscriptEvalInfo)]
    if lib.mh_transcript_eval_plan(*args, int(p2_cycles), -1 if log_n is None else int(log_n), _void_p(row_start), C.byref(info)) != 0:
        raise _plan_refused("mh_transcript_eval_plan", info)
    return row_start, info


def transcript_eval_trace(ctx, p2, nodes, terms, limbs, root, log_n=-1, want_root=True):
    """mh_transcript_eval_trace_build: TranscriptEvalAir's main trace on the device -- `p2` the device-resident Poseidon2 chiplet Trace,
    `nodes` TE_NODE_DTYPE (kind TE_ZERO .. TE_EC_MSM, op, lhs, rhs, perm, ptr, bound_ptr, group, expr) in recording order, `terms`
    TE_TERM_DTYPE (the MSM claims' (base, scalar) node indices), `limbs` uint32 [n_lit, 8] the literal pool, `root` the root's node index
    -> (Trace [., 39], TranscriptEvalInfo, the public root as four ints or None).  Every hash is read from `p2` on the device; value
    nodes' out_mult is counted there.  A refusal raises MidenHipError with `e.info` (kind, index, operand)."""
    keep, args = _te_call_args(nodes, terms, limbs, root)
    lib = ctx.lib
    lib.mh_transcript_eval_trace_build.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t,
                                                   C.c_uint64, C.c_int, C.POINTER(C.c_void_p), C.c_void_p, C.POINTER(TranscriptEvalInfo)]
    h, info, felts = C.c_void_p(), TranscriptEvalInfo(), np.zeros(4, dtype=np.uint64)
    rc = lib.mh_transcript_eval_trace_build(ctx.h, p2.h, *args, -1 if log_n is None else int(log_n), C.byref(h),
                                            felts.ctypes.data_as(C.c_void_p) if want_root else None, C.byref(info))
    _mem_section_result(lib, ctx, rc, info)
    return Trace.from_handle(ctx, h, int(info.rows).bit_length() - 1, 39), info, ([int(x) for x in felts] if want_root else None)


def load_library():
    """dlopen libmidenhip.so (does not touch the GPU)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise MidenHipError(f"{LIB_PATH} is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                            "(there is no CPU fallback)")
    lib = C.CDLL(LIB_PATH)
    lib.mh_last_error.restype = C.c_char_p
    lib.mh_last_error.argtypes = [C.c_void_p]
    lib.mh_ctx_create.argtypes = [C.c_int, C.POINTER(C.c_void_p)]
    lib.mh_ctx_destroy.argtypes = [C.c_void_p]
    lib.mh_trace_free.argtypes = [C.c_void_p]
    lib.mh_tree_free.argtypes = [C.c_void_p]
    lib.mh_tree_log_height.argtypes = [C.c_void_p]
    lib.mh_ctx_set_salt.argtypes = [C.c_void_p, C.c_int, u64p]
    lib.mh_ctx_get_salt.argtypes = [C.c_void_p]
    lib.mh_tree_salt_elems.argtypes = [C.c_void_p]
    lib.mh_tree_salt_index.argtypes = [C.c_void_p]
    lib.mh_tree_salt_index.restype = C.c_uint64
    lib.mh_tree_download_salt.argtypes = [C.c_void_p, C.c_void_p, u64p]
    lib.mh_air_free.argtypes = [C.c_void_p]
    lib.mh_air_log_quotient_degree.argtypes = [C.c_void_p]
    lib.mh_proof_free.argtypes = [C.c_void_p]
    lib.mh_session_free.argtypes = [C.c_void_p]
    lib.mh_pcs_free.argtypes = [C.c_void_p]
    lib.mh_pcs_point_ok.argtypes = [C.c_int, C.c_int, u64p]
    lib.mh_pcs_shape.argtypes = [C.c_void_p, C.c_void_p]
    for name in ("mh_pcs_evals", "mh_pcs_download_deep", "mh_pcs_fri_commit", "mh_pcs_fri_fold", "mh_pcs_fri_final"):
        getattr(lib, name).argtypes = [C.c_void_p, u64p]
    lib.mh_pcs_deep.argtypes = [C.c_void_p, u64p, u64p]
    lib.mh_pcs_query.argtypes = [C.c_void_p, u64p, C.c_size_t, C.POINTER(C.c_void_p)]
    lib.mh_pcs_begin.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_void_p), C.c_int, u64p, C.POINTER(C.c_void_p)]
    lib.mh_pcs_open.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_void_p), C.c_int, u64p, u64p, u64p, C.c_size_t,
                                C.POINTER(C.c_void_p)]
    lib.mh_pcs_verify.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_int, u64p, C.POINTER(C.c_uint8), C.POINTER(C.c_int), C.POINTER(C.c_size_t),
                                  C.c_int, u64p, u64p, u64p, C.c_size_t, u64p, C.c_size_t, u64p, C.c_size_t, u64p, u64p, C.c_char_p, C.c_size_t]
    lib.mh_session_trees.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.c_int, C.POINTER(C.c_int)]
    for name in ("mh_session_shape", "mh_session_commit_main", "mh_session_commit_aux", "mh_session_commit_quotient",
                 "mh_session_ood_point_ok", "mh_session_ood", "mh_session_deep", "mh_session_fri_commit",
                 "mh_session_fri_fold", "mh_session_fri_final", "mh_session_open"):
        getattr(lib, name).restype = C.c_int
    for name in ("mh_proof_num_fields", "mh_proof_num_commitments", "mh_proof_num_traces"):
        getattr(lib, name).restype = C.c_size_t
        getattr(lib, name).argtypes = [C.c_void_p]
    for name in ("mh_proof_fields", "mh_proof_commitments", "mh_proof_digest"):
        getattr(lib, name).restype = u64p
        getattr(lib, name).argtypes = [C.c_void_p]
    lib.mh_proof_log_trace_heights.restype = C.POINTER(C.c_uint8)
    lib.mh_proof_log_trace_heights.argtypes = [C.c_void_p]
    lib.mh_proof_serialize.restype = C.c_size_t
    lib.mh_proof_serialize.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
    _lib = lib
    return lib


def _arr(x):
    return np.ascontiguousarray(np.asarray(x, dtype=np.uint64))


def _ptr(a):
    return a.ctypes.data_as(u64p)


class Ctx:
    """One proving context = one GPU + one private stream (mh_ctx)."""

    def __init__(self, device_id=0):
        self.lib = load_library()
        if self.lib.mh_device_count() <= 0:
            raise MidenHipError("no HIP device visible: libmidenhip has no CPU fallback")
        h = C.c_void_p()
        rc = self.lib.mh_ctx_create(device_id, C.byref(h))
        if rc != 0:
            raise MidenHipError(f"mh_ctx_create failed with code {rc}")
        self.h = h
        self.lmcs_id = 0
        self._children = weakref.WeakSet()  # device objects that must be freed before the ctx

    def check(self, rc):
        if rc != 0:
            raise MidenHipError(f"libmidenhip error {rc}: {self.lib.mh_last_error(self.h).decode()}")

    def close(self):
        if getattr(self, "h", None):
            for child in list(self._children):
                child.free()
            self.lib.mh_ctx_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def ec_traces(self, groups, points, adds, exprs, terms, log_groups=-1, log_points=-1, log_add=-1, log_msm=-1):
        """ec_traces on this context: the session's traces 8..11 (EcGroups, EcPointStore, EcGroupAdd, EcMsm) from the EC ledgers."""
        return ec_traces(self, groups, points, adds, exprs, terms, log_groups, log_points, log_add, log_msm)

    def chunk_node_trace(self, p2, data, digests, records, log_n=-1):
        """chunk_node_trace on this context: the session's trace 0 (ChunkNode) from the node records and the Poseidon2 Trace."""
        return chunk_node_trace(self, p2, data, digests, records, log_n)

    def transcript_eval_trace(self, p2, nodes, terms, limbs, root, log_n=-1, want_root=True):
        """transcript_eval_trace on this context: the session's trace 5 (TranscriptEval) from the transcript's nodes and the Poseidon2 Trace."""
        return transcript_eval_trace(self, p2, nodes, terms, limbs, root, log_n, want_root)

    # ---- profiler ----
    def prof_enable(self, on=True):
        self.check(self.lib.mh_prof_enable(self.h, int(on)))

    def prof_filter(self, name=None):
        """mh_prof_filter: record only this kernel class (None: everything).  Event records are barrier packets: the full
        profile costs a 2^20-row proof ~0.5 ms."""
        self.check(self.lib.mh_prof_filter(self.h, name.encode() if name else None))

    def prof_reset(self):
        self.check(self.lib.mh_prof_reset(self.h))

    def prof(self):
        buf = C.create_string_buffer(1 << 16)
        self.check(self.lib.mh_prof_dump(self.h, buf, C.c_size_t(len(buf))))
        out = {}
        for line in buf.value.decode().splitlines():
            name, ms, by, cnt = line.rsplit(None, 3)  # span names contain blanks
            out[name] = {"ms": float(ms), "bytes": float(by), "count": int(cnt)}
        return out

    def poseidon2_register_rate(self):
        r = C.c_double(0)
        self.check(self.lib.mh_poseidon2_register_rate(self.h, C.byref(r)))
        return r.value

    # ---- unit-parity entry points ----
    def poseidon2_permute(self, states):
        s = _arr(states).copy().reshape(-1, 12)
        self.check(self.lib.mh_poseidon2_permute(self.h, _ptr(s), C.c_size_t(s.shape[0])))
        return s

    def coset_lde_batch(self, matrix, added_bits, shift):
        """Reference storage order: row-major, physical row r = eval at shift*w^bitrev(r)."""
        m = _arr(matrix)
        n, w = m.shape
        log_n = int(n).bit_length() - 1
        assert 1 << log_n == n
        out = np.zeros((n << added_bits, w), dtype=np.uint64)
        self.check(self.lib.mh_coset_lde_batch(self.h, _ptr(m), log_n, C.c_size_t(w), added_bits,
                                               C.c_uint64(int(shift)), _ptr(out)))
        return out

    def trim(self):
        """Release the device buffers pooled between proofs."""
        self.check(self.lib.mh_ctx_trim(self.h))

    def mem_stats(self):
        """(pool bytes, table bytes, device free, device total): what a long-lived service watches (mh_ctx_mem_stats)."""
        out = (C.c_uint64 * 4)()
        self.check(self.lib.mh_ctx_mem_stats(self.h, out))
        return dict(zip(("pool", "tables", "free", "total"), (int(v) for v in out)))

    LMCS = {"poseidon2": 0, "blake3": 1, "keccak": 2, "rpo": 3, "rpx": 4}

    def set_lmcs(self, name):
        """mh_ctx_set_lmcs: the commitment scheme's hasher for commit_traces / tree openings on this context ("poseidon2" |
        "blake3" = the reference's default Blake3_256 configuration, air/src/config.rs:275-289)."""
        self.check(self.lib.mh_ctx_set_lmcs(self.h, self.LMCS[name]))
        self.lmcs_id = self.LMCS[name]

    def set_salt(self, n, seed=None):
        """mh_ctx_set_salt: the hiding LMCS (lmcs/hiding_config.rs) with `n` salt felts per leaf (0 = off) for every tree committed from
        now on.  seed = four integers (reduced mod p) -- secret and fresh per proof -- or None: drawn from the operating system.  Hiding
        commitments alone do not make a proof zero-knowledge (include/midenhip.h)."""
        key = _arr([int(x) % (1 << 64) for x in seed]) if seed is not None else None
        if key is not None and key.size != 4:
            raise MidenHipError("set_salt: the seed is four field elements")
        self.check(self.lib.mh_ctx_set_salt(self.h, C.c_int(int(n)), _ptr(key) if key is not None else None))

    def get_salt(self):
        return int(self.lib.mh_ctx_get_salt(self.h))

    def upload_trace(self, matrix):
        return Trace(self, matrix)


def pinned_array(lib, shape):
    """A numpy uint64 array in page-locked host memory (mh_host_alloc); keep the returned owner alive."""
    n = int(np.prod(shape))
    lib.mh_host_alloc.restype = C.c_void_p
    lib.mh_host_alloc.argtypes = [C.c_size_t]
    lib.mh_host_free.argtypes = [C.c_void_p]
    p = lib.mh_host_alloc(n * 8)
    if not p:
        raise MidenHipError("mh_host_alloc failed")
    buf = (C.c_uint64 * n).from_address(p)
    a = np.frombuffer(buf, dtype=np.uint64).reshape(shape)

    class _Owner:
        def __del__(self, lib=lib, p=p):
            lib.mh_host_free(p)

    return a, _Owner()


class Trace:
    """Device-resident RowMajorMatrix<Felt> (stored column-major on the GPU)."""

    @classmethod
    def from_handle(cls, ctx, h, log_n, width):
        t = cls.__new__(cls)
        t.ctx, t.h, t.log_n, t.width = ctx, h, log_n, width
        ctx._children.add(t)
        return t

    @classmethod
    def from_device(cls, ctx, device_ptr, log_n, width):
        """mh_trace_from_device: wrap a row-major [2^log_n][width] matrix already in device memory."""
        h = C.c_void_p()
        ctx.check(ctx.lib.mh_trace_from_device(ctx.h, C.c_void_p(device_ptr), C.c_int(log_n), C.c_size_t(width), C.byref(h)))
        return cls.from_handle(ctx, h, log_n, width)

    @classmethod
    def upload_async(cls, ctx, pinned_matrix):
        """mh_trace_upload_async: returns at once; the copy runs on the context's copy stream under the compute stream's
        kernels.  `pinned_matrix` (a pinned_array) must stay alive and unmodified until the proof has been made."""
        m = pinned_matrix
        assert m.dtype == np.uint64 and m.flags["C_CONTIGUOUS"] and m.ndim == 2
        n, w = m.shape
        log_n = int(n).bit_length() - 1
        assert 1 << log_n == n, "trace height must be a power of two"
        h = C.c_void_p()
        ctx.check(ctx.lib.mh_trace_upload_async(ctx.h, _ptr(m), log_n, C.c_size_t(w), C.byref(h)))
        t = cls.from_handle(ctx, h, log_n, w)
        t._source = m  # keeps the host buffer alive as long as the trace
        return t

    @classmethod
    def upload_cols_async(cls, ctx, pinned_colmajor):
        """mh_trace_upload_cols_async: `pinned_colmajor` is the TRANSPOSED matrix, shape (width, 2^log_n), C-contiguous (a pinned_array):
        columns go up in groups of eight, the LDE of a group starts when it has landed."""
        m = pinned_colmajor
        assert m.dtype == np.uint64 and m.flags["C_CONTIGUOUS"] and m.ndim == 2
        w, n = m.shape
        log_n = int(n).bit_length() - 1
        assert 1 << log_n == n, "trace height must be a power of two"
        h = C.c_void_p()
        ctx.check(ctx.lib.mh_trace_upload_cols_async(ctx.h, _ptr(m), log_n, C.c_size_t(w), C.byref(h)))
        t = cls.from_handle(ctx, h, log_n, w)
        t._source = m
        return t

    def wait(self):
        self.ctx.check(self.ctx.lib.mh_trace_wait(self.ctx.h, self.h))

    def download(self):
        out = np.zeros((1 << self.log_n, self.width), dtype=np.uint64)
        self.ctx.check(self.ctx.lib.mh_trace_download(self.ctx.h, self.h, _ptr(out)))
        return out

    def __init__(self, ctx, matrix):
        m = _arr(matrix)
        n, w = m.shape
        self.log_n = int(n).bit_length() - 1
        assert 1 << self.log_n == n, "trace height must be a power of two"
        self.width = w
        self.ctx = ctx
        h = C.c_void_p()
        ctx.check(ctx.lib.mh_trace_upload(ctx.h, _ptr(m), self.log_n, C.c_size_t(w), C.byref(h)))
        self.h = h
        ctx._children.add(self)

    def free(self):
        if getattr(self, "h", None):
            self.ctx.lib.mh_trace_free(self.h)
            self.h = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class LmcsTree:
    def __init__(self, ctx, h, widths, log_heights, log_blowup):
        self.ctx, self.h = ctx, h
        ctx._children.add(self)
        self.widths, self.log_heights, self.log_blowup = widths, log_heights, log_blowup
        self.log_height = ctx.lib.mh_tree_log_height(h)
        self.salt_elems = int(ctx.lib.mh_tree_salt_elems(h))   # hiding LMCS: salt felts per leaf (0: an ordinary tree)
        self.salt_index = int(ctx.lib.mh_tree_salt_index(h))   # ... and the tree's number in the salt PRF

    def salt(self):
        """mh_tree_download_salt: the tree's salt matrix [2^log_height, salt_elems], physical (bit-reversed) row order like download_lde."""
        out = np.zeros((1 << self.log_height, self.salt_elems), dtype=np.uint64)
        self.ctx.check(self.ctx.lib.mh_tree_download_salt(self.ctx.h, self.h, _ptr(out)))
        return out

    def root(self):
        r = np.zeros(4, dtype=np.uint64)
        self.ctx.check(self.ctx.lib.mh_tree_root(self.h, _ptr(r)))
        return r

    def prove_batch(self, indices, alignment=8):
        """-> (hinted felts, hinted commitments[k][4]) exactly as streamed into the transcript."""
        idx = _arr(list(indices))
        n = idx.size
        tot_w = sum(((w + alignment - 1) // alignment) * alignment for w in self.widths) + self.salt_elems  # rows + raw salt
        fields = np.zeros(max(1, n * tot_w), dtype=np.uint64)
        commits = np.zeros(max(1, n * self.log_height * 4), dtype=np.uint64)
        nf, nc = C.c_size_t(0), C.c_size_t(0)
        self.ctx.check(self.ctx.lib.mh_tree_open(self.ctx.h, self.h, _ptr(idx), C.c_size_t(n), C.c_size_t(alignment),
                                                 _ptr(fields), C.byref(nf), _ptr(commits), C.byref(nc)))
        return fields[:nf.value].copy(), commits[:nc.value].reshape(-1, 4).copy()

    def opening(self, indices, fields, commitments, alignment=8):
        """The mh_lmcs_opening of what prove_batch(indices, alignment) returned, against this tree's root."""
        return LmcsOpening.make(self.root(), self.log_height, self.widths, alignment, indices, fields, commitments)

    def verify_open(self, indices, fields, commitments, alignment=8):
        """mh_lmcs_verify (host only) of an opening of this tree: (True, "") or (False, reason)."""
        lmcs = {v: k for k, v in Ctx.LMCS.items()}[self.ctx.lib.mh_ctx_get_lmcs(self.ctx.h)]
        return lmcs_verify(self.opening(indices, fields, commitments, alignment), lmcs, self.salt_elems)

    def witness(self, indices, fields, commitments, alignment=8):
        """mh_lmcs_witness (host only) of an opening of this tree: the LmcsWitness; raises MidenHipError with the reason if refused."""
        lmcs = {v: k for k, v in Ctx.LMCS.items()}[self.ctx.lib.mh_ctx_get_lmcs(self.ctx.h)]
        return lmcs_witness(self.opening(indices, fields, commitments, alignment), lmcs, self.salt_elems)

    def download_lde(self, mat):
        rows = 1 << (self.log_heights[mat] + self.log_blowup)
        out = np.zeros((rows, self.widths[mat]), dtype=np.uint64)
        self.ctx.check(self.ctx.lib.mh_tree_download_lde(self.ctx.h, self.h, mat, _ptr(out)))
        return out

    def download_layers(self):
        out = np.zeros(((2 << self.log_height) - 1, 4), dtype=np.uint64)
        self.ctx.check(self.ctx.lib.mh_tree_download_layers(self.ctx.h, self.h, _ptr(out)))
        return out

    def free(self):
        if getattr(self, "h", None):
            self.ctx.lib.mh_tree_free(self.h)
            self.h = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class Committed:
    """Mirror of prover/commit.rs `Committed`: root() + tree()."""

    def __init__(self, tree):
        self._tree = tree

    def root(self):
        return self._tree.root()

    def tree(self):
        return self._tree


def commit_traces(ctx, traces, log_blowup):
    """traces: list of Trace in proof order (ascending height)."""
    n = len(traces)
    arr = (C.c_void_p * n)(*[t.h for t in traces])
    h = C.c_void_p()
    root = np.zeros(4, dtype=np.uint64)
    ctx.check(ctx.lib.mh_commit_traces(ctx.h, n, arr, log_blowup, C.byref(h), _ptr(root)))
    return Committed(LmcsTree(ctx, h, [t.width for t in traces], [t.log_n for t in traces], log_blowup))


# ---- the whole proof (miden_prover::prove_stark -> lifted_stark::prover::prove) ---------------------
AUX_CB = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int, u64p, u64p, u64p)


def commit_host(mats, log_blowup, lmcs="poseidon2"):
    """mh_commit_host (host only, no context): the root commit_traces(ctx, mats, log_blowup).root() gives on a context set to `lmcs`,
    from row-major host matrices in proof order (ascending height) -- how a verifier derives an AIR's preprocessed_root."""
    lib = load_library()
    hs = [np.ascontiguousarray(m, dtype=np.uint64) for m in mats]
    n = len(hs)
    if n < 1 or any(m.ndim != 2 or m.shape[0] < 1 or m.shape[0] & (m.shape[0] - 1) for m in hs):
        raise MidenHipError("commit_host: at least one matrix, each 2-D with a power-of-two number of rows")
    ptrs = (u64p * n)(*[_ptr(m) for m in hs])
    lhs = (C.c_uint8 * n)(*[int(m.shape[0]).bit_length() - 1 for m in hs])
    ws = (C.c_size_t * n)(*[m.shape[1] for m in hs])
    root, err = np.zeros(4, dtype=np.uint64), C.create_string_buffer(512)
    lib.mh_commit_host.argtypes = [C.c_int, C.c_int, C.POINTER(u64p), C.POINTER(C.c_uint8), C.POINTER(C.c_size_t), C.c_int, u64p, C.c_char_p,
                                   C.c_size_t]
    rc = lib.mh_commit_host(Ctx.LMCS[lmcs], n, ptrs, lhs, ws, int(log_blowup), _ptr(root), err, 512)
    if rc != 0:
        raise MidenHipError(f"mh_commit_host failed ({rc}): {err.value.decode()}")
    return root


class PcsParams(C.Structure):
    """mh_pcs_params; defaults = the production parameters of air/src/config.rs:54-67."""
    _fields_ = [(k, C.c_int) for k in ("log_blowup", "log_folding_arity", "log_final_degree", "folding_pow_bits",
                                       "deep_pow_bits", "num_queries", "query_pow_bits")]

    @classmethod
    def production(cls):
        return cls(3, 2, 7, 4, 12, 27, 16)

    @classmethod
    def from_dict(cls, d):
        return cls(*[int(d[k]) for k, _ in cls._fields_])


class DeviceAir:
    """mh_air: a constraint-DAG blob (miden-vm_amd/dag.py) loaded and compiled for the device."""

    def __init__(self, ctx, air):
        self.ctx, self.air = ctx, air
        blob = _arr(air.blob)
        h = C.c_void_p()
        ctx.check(ctx.lib.mh_air_load(ctx.h, _ptr(blob), C.c_size_t(blob.size), C.byref(h)))
        self.h = h
        ctx._children.add(self)
        ctx.lib.mh_air_compiled_chunks.argtypes = [C.c_void_p]
        self.compiled_chunks = int(ctx.lib.mh_air_compiled_chunks(h))
        ctx.lib.mh_air_compiled_max_vgprs.argtypes = [C.c_void_p]
        self.compiled_max_vgprs = int(ctx.lib.mh_air_compiled_max_vgprs(h))
        self._lookup = None

    def attach_preprocessed(self, tree, matrix_index, raw=None):
        """Point this AIR at its preprocessed LDE: matrix `matrix_index` of the setup-time LmcsTree (None detaches);
        raw = the uploaded preprocessed Trace itself, needed only when an attached lookup program reads it."""
        self.ctx.check(self.ctx.lib.mh_air_attach_preprocessed(self.h, tree.h if tree is not None else None, C.c_int(matrix_index),
                                                              raw.h if raw is not None else None))
        self._prep_tree, self._prep_raw = tree, raw

    def attach_lookup(self, dev_lookup):
        """Build this AIR's LogUp aux trace on the device during proofs (None detaches)."""
        self.ctx.check(self.ctx.lib.mh_air_attach_lookup(self.h, dev_lookup.h if dev_lookup is not None else None))
        self._lookup = dev_lookup

    def free(self):
        if getattr(self, "h", None):
            self.ctx.lib.mh_air_free(self.h)
            self.h = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def _as_trace(ctx, m):
    return m if m is None or isinstance(m, Trace) else Trace(ctx, m)


def check_constraints(ctx, dev_air, main, aux=None, preprocessed=None, publics=(), randomness=(), aux_values=(), exact=False):
    """mh_check_constraints: every constraint of `dev_air` (a DeviceAir) on every row of `main` (a Trace or a host matrix).
    aux: the aux trace (2 * aux_width base columns, as DeviceLookup.build_aux makes it); randomness / aux_values: EF pairs.
    -> (entries, failing_rows): the failing constraints (list of CheckEntry, [] when satisfied) and the ascending rows on which any
    constraint fails.  exact=True evaluates every constraint on every row instead of screening the rows with a random fold."""
    lib = ctx.lib
    main, aux, preprocessed = _as_trace(ctx, main), _as_trace(ctx, aux), _as_trace(ctx, preprocessed)
    pub = _arr([int(x) for x in publics] or [0])
    rnd = _arr([int(x) for r in randomness for x in r] or [0])
    av = _arr([int(x) for r in aux_values for x in r] or [0])
    rows = np.zeros((1 << main.log_n) + 1, dtype=np.uint64)

    def call(out, cap, n):
        return lib.mh_check_constraints(ctx.h, dev_air.h, main.h, aux.h if aux is not None else None,
                                        preprocessed.h if preprocessed is not None else None, _ptr(pub), C.c_size_t(len(publics)),
                                        _ptr(rnd), C.c_size_t(len(randomness)), _ptr(av), C.c_size_t(len(aux_values)),
                                        C.c_int(MH_CHECK_EXACT if exact else 0), out, cap, n, _ptr(rows))

    entries = _run_check(ctx, call)
    return entries, [int(x) for x in rows[1:1 + int(rows[0])]]


def constraint_fold(ctx, dev_air, main, aux=None, preprocessed=None, publics=(), randomness=(), aux_values=(), alpha=(1, 0)):
    """mh_constraint_fold (a test and diagnostic entry): the fold F(r) = sum_k alpha^(K-1-k) C_k(r) of `dev_air`'s constraints, computed
    by its own constraint program on the rows of `main` with the screen's selector values (is_first = [r == 0], is_last = [r == n-1],
    is_transition = w_n^r - w_n^-1).  Arguments as check_constraints; alpha: an EF pair.  -> ndarray[n, 2] of canonical felts."""
    main, aux, preprocessed = _as_trace(ctx, main), _as_trace(ctx, aux), _as_trace(ctx, preprocessed)
    pub = _arr([int(x) for x in publics] or [0])
    rnd = _arr([int(x) for r in randomness for x in r] or [0])
    av = _arr([int(x) for r in aux_values for x in r] or [0])
    al = _arr([int(alpha[0]), int(alpha[1])])
    out = np.zeros((1 << main.log_n, 2), dtype=np.uint64)
    ctx.check(ctx.lib.mh_constraint_fold(ctx.h, dev_air.h, main.h, aux.h if aux is not None else None,
                                         preprocessed.h if preprocessed is not None else None, _ptr(pub), C.c_size_t(len(publics)),
                                         _ptr(rnd), C.c_size_t(len(randomness)), _ptr(av), C.c_size_t(len(aux_values)), _ptr(al), _ptr(out)))
    return out


class DeviceLookup:
    """mh_lookup: a LogUp lookup program ("MHLKP001" blob, dag.LookupBuilder) compiled for the device."""

    def __init__(self, ctx, lookup):
        self.ctx, self.lookup = ctx, lookup
        blob = _arr(lookup.blob)
        h = C.c_void_p()
        ctx.lib.mh_lookup_free.argtypes = [C.c_void_p]
        ctx.check(ctx.lib.mh_lookup_load(ctx.h, _ptr(blob), C.c_size_t(blob.size), C.byref(h)))
        self.h = h
        ctx._children.add(self)

    def build_aux(self, main_trace, randomness, preprocessed=None):
        """-> (aux Trace on the device [n, 2 * (num_cols + registers)], (c0, c1) accumulator final)."""
        rnd = _arr([int(x) for r in randomness for x in r] or [0])
        h = C.c_void_p()
        fin = np.zeros(2, dtype=np.uint64)
        self.ctx.check(self.ctx.lib.mh_lookup_build_aux(self.ctx.h, self.h, main_trace.h, preprocessed.h if preprocessed is not None else None,
                                                        _ptr(rnd), C.c_size_t(len(randomness)),
                                                        C.byref(h), _ptr(fin)))
        return Trace.from_handle(self.ctx, h, main_trace.log_n, 2 * self.lookup.num_aux_cols), (int(fin[0]), int(fin[1]))

    def free(self):
        if getattr(self, "h", None):
            self.ctx.lib.mh_lookup_free(self.h)
            self.h = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class Proof:
    """StarkProofData + digest (crates/lifted-stark/src/proof.rs:58-63)."""

    def __init__(self, lib, h):
        nf, nc, nt = lib.mh_proof_num_fields(h), lib.mh_proof_num_commitments(h), lib.mh_proof_num_traces(h)
        # an empty vector's data pointer may be null (mh_session_open of a statement whose openings need no sibling: every path node is
        # an ancestor of another query) -- found by tests/test_gpu_fuzz_parity.py
        self.fields = np.ctypeslib.as_array(lib.mh_proof_fields(h), shape=(nf,)).copy() if nf else np.zeros(0, dtype=np.uint64)
        self.commitments = (np.ctypeslib.as_array(lib.mh_proof_commitments(h), shape=(nc * 4,)).copy() if nc else np.zeros(0, dtype=np.uint64)).reshape(-1, 4)
        self.digest = np.ctypeslib.as_array(lib.mh_proof_digest(h), shape=(4,)).copy()
        lh = lib.mh_proof_log_trace_heights(h)
        self.log_trace_heights = [int(lh[i]) for i in range(nt)]
        need = lib.mh_proof_serialize(h, None, 0)
        buf = (C.c_uint8 * need)()
        lib.mh_proof_serialize(h, buf, need)
        self.bytes = bytes(buf)
        lib.mh_proof_free(h)


def proof_from_bytes(data):
    """mh_proof_deserialize (host only): StarkProofData bytes -> Proof (digest zeroed); raises MidenHipError on malformed input."""
    lib = load_library()
    buf = (C.c_uint8 * max(1, len(data))).from_buffer_copy(bytes(data) or b"\0")
    h = C.c_void_p()
    lib.mh_proof_deserialize.argtypes = [C.c_void_p, C.c_size_t, C.POINTER(C.c_void_p)]
    rc = lib.mh_proof_deserialize(buf, C.c_size_t(len(data)), C.byref(h))
    if rc != 0:
        raise MidenHipError(f"mh_proof_deserialize failed ({rc}): malformed StarkProofData bytes")
    return Proof(lib, h)


def prove(ctx, airs, traces, public_values, params, challenger_state, pre_observe, aux_builder=None):
    """airs: list of DeviceAir, traces: list of Trace (instance order).  aux_builder: None (all-zero aux
    traces, DummyMidenAir) or a Python callable (instance_idx, randomness[(c0,c1)...]) ->
    (aux[n, 2*aux_width] uint64, flat aux values)."""
    n = len(airs)
    a_arr = (C.c_void_p * n)(*[a.h for a in airs])
    t_arr = (C.c_void_p * n)(*[t.h for t in traces])
    pub = _arr(list(public_values) or [0])
    st = _arr(challenger_state)
    pre = _arr(list(pre_observe) or [0])
    max_rand = max(a.air.num_randomness for a in airs)

    def cb(user, idx, rand_p, aux_p, vals_p):
        try:
            rnd = [(int(rand_p[2 * i]), int(rand_p[2 * i + 1])) for i in range(max_rand)]
            aux, vals = aux_builder(idx, rnd)
            flat = np.ascontiguousarray(aux, dtype=np.uint64).reshape(-1)
            C.memmove(aux_p, flat.ctypes.data, flat.size * 8)
            for i, v in enumerate(vals):
                vals_p[i] = int(v)
            return 0
        except Exception as e:  # pragma: no cover
            print("aux builder failed:", e)
            return 1

    c_cb = AUX_CB(cb) if aux_builder is not None else C.cast(None, AUX_CB)
    h = C.c_void_p()
    p = params if isinstance(params, PcsParams) else PcsParams.from_dict(params)
    ctx.check(ctx.lib.mh_prove(ctx.h, C.byref(p), C.c_int(n), a_arr, t_arr, _ptr(pub), C.c_size_t(len(public_values)),
                               _ptr(st), _ptr(pre), C.c_size_t(len(pre_observe)), c_cb, None, C.byref(h)))
    return Proof(ctx.lib, h)


def prove_host(ctx, airs, host_traces, public_values, params, challenger_state, pre_observe, aux_builder=None):
    """mh_prove_host: `host_traces` = row-major uint64 matrices in HOST memory (pinned_array for full overlap), instance order.
    The uploads run inside the call, overlapped with the proof (matrix k + 1 lands under matrix k's LDE and leaf sponges)."""
    n = len(airs)
    a_arr = (C.c_void_p * n)(*[a.h for a in airs])
    mats = [m if (m.dtype == np.uint64 and m.flags["C_CONTIGUOUS"]) else _arr(m) for m in host_traces]
    t_arr = (u64p * n)(*[_ptr(m) for m in mats])
    lhs = (C.c_int * n)(*[int(m.shape[0]).bit_length() - 1 for m in mats])
    for m, a in zip(mats, airs):
        assert m.ndim == 2 and m.shape[1] == a.air.main_width and 1 << (int(m.shape[0]).bit_length() - 1) == m.shape[0]
    pub, st, pre = _arr(list(public_values) or [0]), _arr(challenger_state), _arr(list(pre_observe) or [0])
    c_cb = _aux_callback(aux_builder, max(a.air.num_randomness for a in airs))
    h = C.c_void_p()
    p = params if isinstance(params, PcsParams) else PcsParams.from_dict(params)
    ctx.check(ctx.lib.mh_prove_host(ctx.h, C.byref(p), C.c_int(n), a_arr, t_arr, lhs, _ptr(pub), C.c_size_t(len(public_values)), _ptr(st),
                                    _ptr(pre), C.c_size_t(len(pre_observe)), c_cb, None, C.byref(h)))
    return Proof(ctx.lib, h)


def _aux_callback(aux_builder, max_rand):
    if aux_builder is None:
        return C.cast(None, AUX_CB)

    def cb(user, idx, rand_p, aux_p, vals_p):
        try:
            rnd = [(int(rand_p[2 * i]), int(rand_p[2 * i + 1])) for i in range(max_rand)]
            aux, vals = aux_builder(idx, rnd)
            flat = np.ascontiguousarray(aux, dtype=np.uint64).reshape(-1)
            C.memmove(aux_p, flat.ctypes.data, flat.size * 8)
            for i, v in enumerate(vals):
                vals_p[i] = int(v)
            return 0
        except Exception as e:  # pragma: no cover
            print("aux builder failed:", e)
            return 1

    return AUX_CB(cb)


class SessionShape(C.Structure):
    _fields_ = [("log_lde_height", C.c_int), ("num_randomness", C.c_size_t), ("num_aux_values", C.c_size_t),
                ("ood_width", C.c_size_t), ("num_fri_rounds", C.c_int), ("final_poly_len", C.c_size_t)]


class Session:
    """mh_session: the device stages of one proof, driven by a caller-owned transcript
    (ProverInstance::prove, crates/lifted-stark/src/prover/mod.rs:230-578, one method per step).
    EF values are (c0, c1) tuples."""

    def __init__(self, ctx, airs, traces, public_values, params, comm=None):
        self.ctx, self.lib = ctx, ctx.lib
        self._keep = (list(airs), list(traces))  # the session borrows them until it is freed
        n = len(airs)
        a_arr = (C.c_void_p * n)(*[a.h for a in airs])
        t_arr = (C.c_void_p * n)(*[t.h for t in traces])
        pub = _arr(list(public_values) or [0])
        self.params = params if isinstance(params, PcsParams) else PcsParams.from_dict(params)
        h = C.c_void_p()
        ctx.check(self.lib.mh_session_begin(ctx.h, C.byref(comm) if comm is not None else None, C.byref(self.params), C.c_int(n),
                                            a_arr, t_arr, _ptr(pub), C.c_size_t(len(public_values)), C.byref(h)))
        self.h = h
        ctx._children.add(self)
        self.shape = SessionShape()
        ctx.check(self.lib.mh_session_shape(self.h, C.byref(self.shape)))

    @staticmethod
    def _e(v):
        return _arr([int(v[0]), int(v[1])])

    def _root(self, fn, *args):
        root = np.zeros(4, dtype=np.uint64)
        self.ctx.check(fn(self.h, *args, _ptr(root)))
        return root

    def commit_main(self):
        return self._root(self.lib.mh_session_commit_main)

    def commit_aux(self, randomness, aux_builder=None):
        """-> (root, aux values as a flat uint64 array [2 * num_aux_values], proof order)."""
        rnd = _arr([int(x) for r in randomness for x in r] or [0])
        vals = np.zeros(max(1, 2 * self.shape.num_aux_values), dtype=np.uint64)
        cb = _aux_callback(aux_builder, self.shape.num_randomness)
        root = np.zeros(4, dtype=np.uint64)
        self.ctx.check(self.lib.mh_session_commit_aux(self.h, _ptr(rnd), cb, None, _ptr(root), _ptr(vals)))
        return root, vals[:2 * self.shape.num_aux_values]

    def commit_quotient(self, alpha, beta):
        a, b = self._e(alpha), self._e(beta)
        return self._root(self.lib.mh_session_commit_quotient, _ptr(a), _ptr(b))

    def ood_point_ok(self, z):
        zz = self._e(z)
        return bool(self.lib.mh_session_ood_point_ok(self.h, _ptr(zz)))

    def ood(self, z):
        """-> flat uint64 [2 * 2 * ood_width]: the row at z, then the row at z * w_H."""
        zz = self._e(z)
        out = np.zeros(4 * self.shape.ood_width, dtype=np.uint64)
        self.ctx.check(self.lib.mh_session_ood(self.h, _ptr(zz), _ptr(out)))
        return out

    def deep(self, alpha, beta):
        a, b = self._e(alpha), self._e(beta)
        self.ctx.check(self.lib.mh_session_deep(self.h, _ptr(a), _ptr(b)))

    def fri_commit(self):
        return self._root(self.lib.mh_session_fri_commit)

    def fri_fold(self, beta):
        b = self._e(beta)
        self.ctx.check(self.lib.mh_session_fri_fold(self.h, _ptr(b)))

    def fri_final(self):
        out = np.zeros(2 * self.shape.final_poly_len, dtype=np.uint64)
        self.ctx.check(self.lib.mh_session_fri_final(self.h, _ptr(out)))
        return out

    def open(self, indices):
        """-> Proof carrying only the hinted fields / commitments."""
        idx = _arr([int(i) for i in indices])
        h = C.c_void_p()
        self.ctx.check(self.lib.mh_session_open(self.h, _ptr(idx), C.c_size_t(idx.size), C.byref(h)))
        return Proof(self.lib, h)

    def trees(self):
        """mh_session_trees: the session's input trees in group order [preprocessed?, main, aux, quotient] as raw handles (c_void_p),
        BORROWED -- valid until the session is freed, never to be freed by the caller; for PcsOpening / pcs_open.  Available once the
        quotient is committed."""
        arr, n = (C.c_void_p * 8)(), C.c_int(0)
        self.ctx.check(self.lib.mh_session_trees(self.h, arr, 8, C.byref(n)))
        return [C.c_void_p(arr[i]) for i in range(n.value)]

    def free(self):
        if getattr(self, "h", None):
            self.lib.mh_session_free(self.h)
            self.h = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


# ---- the polynomial commitment scheme on its own (pcs::open_with_channel / pcs::verify_aligned) ----------------
class PcsShape(C.Structure):
    _fields_ = [("log_lde_height", C.c_int), ("n_points", C.c_int), ("ood_width", C.c_size_t), ("num_fri_rounds", C.c_int),
                ("final_poly_len", C.c_size_t)]


def _tree_handles(trees):
    """LmcsTree / Committed objects or raw handles (Session.trees()) -> a C array of mh_tree*."""
    hs = []
    for t in trees:
        t = t.tree() if isinstance(t, Committed) else t
        hs.append(t.h if isinstance(t, LmcsTree) else t)
    return (C.c_void_p * max(1, len(hs)))(*hs)


def _points(points):
    return _arr([int(x) for z in points for x in z] or [0])


def pcs_point_ok(log_max_trace_height, log_blowup, z):
    """mh_pcs_point_ok (host only): z = (c0, c1) is nonzero, outside the trace domain H of the tallest matrix and outside the LDE coset gK."""
    zz = _arr([int(z[0]), int(z[1])])
    return bool(load_library().mh_pcs_point_ok(int(log_max_trace_height), int(log_blowup), _ptr(zz)))


class PcsOpening:
    """mh_pcs: committed trees opened at 1..4 points, one method per step of pcs::open_with_channel (crates/lifted-stark/src/pcs/
    prover.rs:34-101), for a caller-owned transcript.  trees: LmcsTree / Committed objects (or Session.trees() handles), borrowed for
    the opening's lifetime; points: [(c0, c1), ...].  EF values are (c0, c1) tuples."""

    def __init__(self, ctx, trees, points, params):
        self.ctx, self.lib = ctx, ctx.lib
        self._keep = list(trees)
        self.params = params if isinstance(params, PcsParams) else PcsParams.from_dict(params)
        pts = _points(points)
        h = C.c_void_p()
        ctx.check(self.lib.mh_pcs_begin(ctx.h, C.byref(self.params), len(self._keep), _tree_handles(self._keep), len(points), _ptr(pts),
                                        C.byref(h)))
        self.h = h
        ctx._children.add(self)
        self.shape = PcsShape()
        ctx.check(self.lib.mh_pcs_shape(self.h, C.byref(self.shape)))

    def evals(self):
        """-> uint64 [n_points, ood_width, 2]: per point the aligned evaluations of every matrix of every tree, transcript order."""
        out = np.zeros((self.shape.n_points, self.shape.ood_width, 2), dtype=np.uint64)
        self.ctx.check(self.lib.mh_pcs_evals(self.h, _ptr(out)))
        return out

    def deep(self, alpha, beta):
        a, b = Session._e(alpha), Session._e(beta)
        self.ctx.check(self.lib.mh_pcs_deep(self.h, _ptr(a), _ptr(b)))

    def download_deep(self):
        """-> uint64 [2^log_lde_height, 2]: the DEEP layer in domain order (index i <-> x = g * w_K^i)."""
        out = np.zeros((1 << self.shape.log_lde_height, 2), dtype=np.uint64)
        self.ctx.check(self.lib.mh_pcs_download_deep(self.h, _ptr(out)))
        return out

    def fri_commit(self):
        root = np.zeros(4, dtype=np.uint64)
        self.ctx.check(self.lib.mh_pcs_fri_commit(self.h, _ptr(root)))
        return root

    def fri_fold(self, beta):
        b = Session._e(beta)
        self.ctx.check(self.lib.mh_pcs_fri_fold(self.h, _ptr(b)))

    def fri_final(self):
        out = np.zeros(2 * self.shape.final_poly_len, dtype=np.uint64)
        self.ctx.check(self.lib.mh_pcs_fri_final(self.h, _ptr(out)))
        return out

    def query(self, indices):
        """-> Proof carrying only the hinted fields / commitments (every input tree in order, then every FRI round)."""
        idx = _arr([int(i) for i in indices])
        h = C.c_void_p()
        self.ctx.check(self.lib.mh_pcs_query(self.h, _ptr(idx), C.c_size_t(idx.size), C.byref(h)))
        return Proof(self.lib, h)

    def free(self):
        if getattr(self, "h", None):
            self.lib.mh_pcs_free(self.h)
            self.h = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def pcs_open(ctx, trees, points, params, challenger_state, pre_observe):
    """mh_pcs_open: the whole opening with the library's transcript -> Proof (fields, commitments, digest).  The roots are NOT observed
    by the library: put them into pre_observe (four words per root), here and in pcs_verify."""
    keep = list(trees)
    p = params if isinstance(params, PcsParams) else PcsParams.from_dict(params)
    pts, st, pre = _points(points), _arr(challenger_state), _arr(list(pre_observe) or [0])
    h = C.c_void_p()
    ctx.check(ctx.lib.mh_pcs_open(ctx.h, C.byref(p), len(keep), _tree_handles(keep), len(points), _ptr(pts), _ptr(st), _ptr(pre),
                                  C.c_size_t(len(pre_observe)), C.byref(h)))
    return Proof(ctx.lib, h)


def pcs_verify(roots, log_tree_heights, widths, points, params, challenger_state, pre_observe, fields, commitments, lmcs="poseidon2",
               salt_elems=0):
    """mh_pcs_verify (host only, no GPU): roots[t] = tree t's four words, log_tree_heights[t] = log2 rows of its tallest matrix,
    widths[t] = the unpadded widths of its matrices.  Returns (True, digest, evals uint64 [n_points, sum of widths, 2]) or
    (False, message, None)."""
    lib = load_library()
    n = len(roots)
    r = _arr(np.asarray(roots, dtype=np.uint64).reshape(-1) if n else [0])
    lh = (C.c_uint8 * max(1, n))(*[int(x) for x in log_tree_heights])
    nm = (C.c_int * max(1, n))(*[len(w) for w in widths])
    flat = [int(w) for ws in widths for w in ws]
    ws = (C.c_size_t * max(1, len(flat)))(*flat)
    p = params if isinstance(params, PcsParams) else PcsParams.from_dict(params)
    pts, st, pre = _points(points), _arr(challenger_state), _arr(list(pre_observe) or [0])
    f = _arr(fields if len(fields) else [0])
    cm = _arr(np.asarray(commitments, dtype=np.uint64).reshape(-1))
    cm = cm if cm.size else _arr([0])
    n_cm = np.asarray(commitments).size // 4
    ok_n = 1 <= len(points) <= MH_PCS_MAX_POINTS
    evals = np.zeros((len(points) if ok_n else 1, max(1, sum(flat)), 2), dtype=np.uint64)
    digest, err = np.zeros(4, dtype=np.uint64), C.create_string_buffer(512)
    rc = lib.mh_pcs_verify(Ctx.LMCS[lmcs], int(salt_elems), C.byref(p), n, _ptr(r), lh, nm, ws, len(points), _ptr(pts), _ptr(st), _ptr(pre),
                           C.c_size_t(len(pre_observe)), _ptr(f), C.c_size_t(len(fields)), _ptr(cm), C.c_size_t(n_cm), _ptr(evals),
                           _ptr(digest), err, C.c_size_t(512))
    if rc != 0:
        return False, err.value.decode(), None
    return True, digest, evals[:, :sum(flat)]


def grind(ctx, state, pending, bits):
    """mh_grind: smallest PoW witness for the challenger (state[12], pending absorbed felts)."""
    st, pe = _arr(state), _arr(list(pending) or [0])
    w = C.c_uint64(0)
    ctx.check(ctx.lib.mh_grind(ctx.h, _ptr(st), _ptr(pe), C.c_size_t(len(pending)), C.c_int(bits), C.byref(w)))
    return int(w.value)


EXTERNAL_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.POINTER(C.c_uint64), C.c_size_t, C.POINTER(C.POINTER(C.c_uint64)),
                          C.POINTER(C.c_size_t), C.POINTER(C.c_uint8), C.c_int, C.POINTER(C.c_uint64), C.c_size_t)


def external_callback(fn):
    """Wrap a Python function (randomness[(c0,c1)], aux_values[instance][(c0,c1)], log_heights) -> [(c0,c1), ...] as an
    mh_external_assertions callback (Statement::eval_external, see midenhip.h).  Raising = ReductionError."""
    def raw(_user, rnd, n_rnd, aux, n_aux, lhs, n_airs, out, cap):
        try:
            r = [(int(rnd[2 * i]), int(rnd[2 * i + 1])) for i in range(n_rnd)]
            av = [[(int(aux[i][2 * k]), int(aux[i][2 * k + 1])) for k in range(n_aux[i])] for i in range(n_airs)]
            vals = fn(r, av, [int(lhs[i]) for i in range(n_airs)])
            if len(vals) > cap:
                return -1
            for k, (a, b) in enumerate(vals):
                out[2 * k], out[2 * k + 1] = int(a), int(b)
            return len(vals)
        except Exception:
            return -1
    return EXTERNAL_FN(raw)


def verify(airs, log_trace_heights, public_values, params, challenger_state, pre_observe, fields, commitments,
           preprocessed_root=None, external=None, lmcs="poseidon2", salt_elems=0):
    """mh_verify / mh_verify_ex (host only, no GPU): airs = dag.Air objects in instance order; preprocessed_root = the setup
    commitment when some AIR has preprocessed columns (it must also be in pre_observe); external = the statement's cross-AIR
    assertions: an EXTERNAL_FN / external_callback(...) object, the string "logup_balance" for the library's
    mh_external_logup_balance, or "precompile_session" / "precompile_session_ec_only" for its mh_external_precompile_session.
    salt_elems > 0: mh_verify_hiding, for a proof made after Ctx.set_salt(salt_elems).  Returns (ok, digest or message)."""
    lib = load_library()
    n = len(airs)
    blobs = [_arr(a.blob) for a in airs]
    bp = (u64p * n)(*[_ptr(b) for b in blobs])
    bl = (C.c_size_t * n)(*[b.size for b in blobs])
    lh = (C.c_uint8 * n)(*[int(x) for x in log_trace_heights])
    pub, st, pre = _arr(list(public_values) or [0]), _arr(challenger_state), _arr(list(pre_observe) or [0])
    f = _arr(fields)
    c = _arr(np.asarray(commitments, dtype=np.uint64).reshape(-1))
    p = params if isinstance(params, PcsParams) else PcsParams.from_dict(params)
    digest = np.zeros(4, dtype=np.uint64)
    err = C.create_string_buffer(512)
    proot = _arr(preprocessed_root) if preprocessed_root is not None else None
    ext_user = None
    if external in ("precompile_session", "precompile_session_ec_only"):   # the library's ChipletMultiAir::eval_external (session/prove.rs:243-256)
        external = C.cast(lib.mh_external_precompile_session_ec_only if external.endswith("ec_only") else lib.mh_external_precompile_session, EXTERNAL_FN)
    if salt_elems:  # mh_verify_hiding: any configuration, `rows + salt` per opened leaf
        ext = C.cast(lib.mh_external_logup_balance, EXTERNAL_FN) if external == "logup_balance" else external
        rc = lib.mh_verify_hiding(C.c_int(Ctx.LMCS[lmcs]), C.c_int(int(salt_elems)), C.byref(p), C.c_int(n), bp, bl, lh, _ptr(pub),
                                  C.c_size_t(len(public_values)), _ptr(st), _ptr(pre), C.c_size_t(len(pre_observe)), _ptr(f),
                                  C.c_size_t(f.size), _ptr(c), C.c_size_t(c.size // 4), _ptr(proot) if proot is not None else None,
                                  ext if ext is not None else C.cast(None, EXTERNAL_FN), ext_user, _ptr(digest), err, C.c_size_t(512))
    elif lmcs != "poseidon2":  # mh_verify_lmcs: the other algebraic configurations ("rpo", "rpx")
        ext = C.cast(lib.mh_external_logup_balance, EXTERNAL_FN) if external == "logup_balance" else external
        rc = lib.mh_verify_lmcs(C.c_int(Ctx.LMCS[lmcs]), C.byref(p), C.c_int(n), bp, bl, lh, _ptr(pub), C.c_size_t(len(public_values)),
                                _ptr(st), _ptr(pre), C.c_size_t(len(pre_observe)), _ptr(f), C.c_size_t(f.size), _ptr(c),
                                C.c_size_t(c.size // 4), _ptr(proot) if proot is not None else None,
                                ext if ext is not None else C.cast(None, EXTERNAL_FN), ext_user, _ptr(digest), err, C.c_size_t(512))
    elif external is None:
        rc = lib.mh_verify(C.byref(p), C.c_int(n), bp, bl, lh, _ptr(pub), C.c_size_t(len(public_values)), _ptr(st), _ptr(pre),
                           C.c_size_t(len(pre_observe)), _ptr(f), C.c_size_t(f.size), _ptr(c), C.c_size_t(c.size // 4),
                           _ptr(proot) if proot is not None else None, _ptr(digest), err, C.c_size_t(512))
    else:
        ext = C.cast(lib.mh_external_logup_balance, EXTERNAL_FN) if external == "logup_balance" else external
        rc = lib.mh_verify_ex(C.byref(p), C.c_int(n), bp, bl, lh, _ptr(pub), C.c_size_t(len(public_values)), _ptr(st), _ptr(pre),
                              C.c_size_t(len(pre_observe)), _ptr(f), C.c_size_t(f.size), _ptr(c), C.c_size_t(c.size // 4),
                              _ptr(proot) if proot is not None else None, ext, ext_user, _ptr(digest), err, C.c_size_t(512))
    return (True, digest) if rc == 0 else (False, err.value.decode())


# ---- LMCS openings on their own and the batch verifier (csrc/lmcs_verify.cpp, csrc/verify_batch.hip) ---------------------------------
class LmcsOpening(C.Structure):
    """mh_lmcs_opening; make() keeps the arrays it points to alive."""
    _fields_ = [("root", C.c_uint64 * 4), ("log_height", C.c_int), ("n_mats", C.c_int), ("widths", C.POINTER(C.c_size_t)),
                ("alignment", C.c_size_t), ("indices", u64p), ("n_indices", C.c_size_t), ("fields", u64p), ("n_fields", C.c_size_t),
                ("commitments", u64p), ("n_commit_felts", C.c_size_t)]

    @classmethod
    def make(cls, root, log_height, widths, alignment, indices, fields, commitments):
        o = cls()
        w = (C.c_size_t * max(1, len(widths)))(*[int(x) for x in widths])
        idx, f = _arr([int(i) for i in indices]), _arr(fields)
        c = _arr(np.asarray(commitments, dtype=np.uint64).reshape(-1))
        o._keep = (w, idx, f, c)
        o.root = (C.c_uint64 * 4)(*[int(x) for x in root])
        o.log_height, o.n_mats, o.widths, o.alignment = int(log_height), len(widths), w, int(alignment)
        o.indices, o.n_indices = (_ptr(idx) if idx.size else None), idx.size
        o.fields, o.n_fields = (_ptr(f) if f.size else None), f.size
        o.commitments, o.n_commit_felts = (_ptr(c) if c.size else None), c.size
        return o


def _openings(openings):
    items = [o if isinstance(o, LmcsOpening) else LmcsOpening.make(**o) for o in openings]
    arr = (LmcsOpening * max(1, len(items)))(*items)
    return items, arr


def lmcs_verify(opening, lmcs="poseidon2", salt_elems=0):
    """mh_lmcs_verify (host only): opening = an LmcsOpening or the keyword arguments of LmcsOpening.make as a dict.
    Returns (True, "") or (False, reason)."""
    lib = load_library()
    items, arr = _openings([opening])
    err = C.create_string_buffer(512)
    lib.mh_lmcs_verify.argtypes = [C.c_int, C.c_int, C.POINTER(LmcsOpening), C.c_char_p, C.c_size_t]
    rc = lib.mh_lmcs_verify(Ctx.LMCS[lmcs], int(salt_elems), arr, err, 512)
    return (rc == 0, err.value.decode())


def lmcs_verify_batch(ctx, openings, lmcs="poseidon2", salt_elems=0):
    """mh_lmcs_verify_batch: the openings hashed on the device; returns the list of 0/1 verdicts."""
    items, arr = _openings(openings)
    ok = (C.c_int * max(1, len(items)))()
    ctx.lib.mh_lmcs_verify_batch.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_size_t, C.POINTER(LmcsOpening), C.POINTER(C.c_int)]
    ctx.check(ctx.lib.mh_lmcs_verify_batch(ctx.h, Ctx.LMCS[lmcs], int(salt_elems), len(items), arr, ok))
    return [int(ok[i]) for i in range(len(items))]


# ---- openings read back as Merkle witnesses (mh_lmcs_witness*, mh_verify_batch_witness) ---------------------------------------------
class LmcsWitness:
    """What the verifier of one opening derives: indices (sorted, unique), leaf_digests[k][4], paths[k][depth][4], nodes[n_nodes][4]
    (None if not asked for).  path(i) = the authentication path of opened leaf i, bottom to top; root() = the derived root."""

    def __init__(self, indices, leaf_digests, paths, nodes):
        self.indices, self.leaf_digests, self.paths, self.nodes = indices, leaf_digests, paths, nodes

    @property
    def depth(self):
        return self.paths.shape[1]

    def path(self, i):
        q = int(np.searchsorted(self.indices, np.uint64(i)))
        if q >= self.indices.size or int(self.indices[q]) != int(i):
            raise KeyError(f"leaf {i} is not opened")
        return self.paths[q]

    def root(self):
        if self.depth == 0:
            return self.leaf_digests[0]
        if self.nodes is None:
            raise MidenHipError("LmcsWitness.root: the witness was made without its nodes")
        return self.nodes[-1]


class LmcsWitnessOut(C.Structure):
    _fields_ = [("leaf_digests", u64p), ("paths", u64p), ("nodes", u64p)]


def lmcs_witness_size(opening):
    """mh_lmcs_witness_size: (n_leaves, n_nodes) of the witness of an opening (only its height and indices are read)."""
    lib = load_library()
    items, arr = _openings([opening])
    k, m, err = C.c_size_t(0), C.c_size_t(0), C.create_string_buffer(512)
    lib.mh_lmcs_witness_size.argtypes = [C.POINTER(LmcsOpening), C.POINTER(C.c_size_t), C.POINTER(C.c_size_t), C.c_char_p, C.c_size_t]
    if lib.mh_lmcs_witness_size(arr, C.byref(k), C.byref(m), err, 512) != 0:
        raise MidenHipError(err.value.decode())
    return k.value, m.value


def _witness_buffers(o, nodes=True):
    k, m = lmcs_witness_size(o)
    idx = np.unique(np.array([int(o.indices[i]) for i in range(o.n_indices)], dtype=np.uint64))
    return LmcsWitness(idx, np.zeros((k, 4), dtype=np.uint64), np.zeros((k, o.log_height, 4), dtype=np.uint64),
                       np.zeros((m, 4), dtype=np.uint64) if nodes else None)


def lmcs_witness(opening, lmcs="poseidon2", salt_elems=0, nodes=True):
    """mh_lmcs_witness (host only): the LmcsWitness of an opening mh_lmcs_verify accepts; MidenHipError with its reason otherwise."""
    lib = load_library()
    items, arr = _openings([opening])
    w = _witness_buffers(items[0], nodes)
    err = C.create_string_buffer(512)
    lib.mh_lmcs_witness.argtypes = [C.c_int, C.c_int, C.POINTER(LmcsOpening), C.c_void_p, C.c_void_p, C.c_void_p, C.c_char_p, C.c_size_t]
    rc = lib.mh_lmcs_witness(Ctx.LMCS[lmcs], int(salt_elems), arr, w.leaf_digests.ctypes.data, w.paths.ctypes.data,
                             w.nodes.ctypes.data if nodes else None, err, 512)
    if rc != 0:
        raise MidenHipError(err.value.decode())
    return w


def lmcs_witness_batch(ctx, openings, lmcs="poseidon2", salt_elems=0, nodes=True):
    """mh_lmcs_witness_batch: the openings hashed on the device and read back as witnesses; per opening its LmcsWitness, or None
    where mh_lmcs_witness refuses it."""
    items, arr = _openings(openings)
    ws = []
    for o in items:
        try:
            ws.append(_witness_buffers(o, nodes))
        except MidenHipError:  # an index the shape check refuses: the call itself gives the verdict 0, its buffers are never written
            ws.append(LmcsWitness(np.zeros(0, dtype=np.uint64), np.zeros((1, 4), dtype=np.uint64), np.zeros((1, 1, 4), dtype=np.uint64), None))
    outs = (LmcsWitnessOut * max(1, len(items)))()
    for k, w in enumerate(ws):
        outs[k].leaf_digests, outs[k].paths = _ptr(w.leaf_digests), C.cast(w.paths.ctypes.data, u64p)
        outs[k].nodes = _ptr(w.nodes) if w.nodes is not None and w.nodes.size else None
    ok = (C.c_int * max(1, len(items)))()
    ctx.lib.mh_lmcs_witness_batch.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_size_t, C.POINTER(LmcsOpening), C.POINTER(LmcsWitnessOut),
                                              C.POINTER(C.c_int)]
    ctx.check(ctx.lib.mh_lmcs_witness_batch(ctx.h, Ctx.LMCS[lmcs], int(salt_elems), len(items), arr, outs, ok))
    return [w if ok[k] else None for k, w in enumerate(ws)]


class WitnessTreeView(C.Structure):
    _fields_ = [("kind", C.c_int), ("which", C.c_int), ("depth", C.c_int), ("n_leaves", C.c_size_t), ("n_nodes", C.c_size_t),
                ("row_len", C.c_size_t), ("root", C.c_uint64 * 4), ("indices", u64p), ("rows", u64p), ("leaf_digests", u64p), ("paths", u64p),
                ("nodes", u64p)]


class WitnessTree(LmcsWitness):
    """One tree of a verified proof (mh_witness_tree), copied out of the set: an LmcsWitness plus kind (0 committed, 1 FRI round),
    which, tree_root (the proof's commitment) and rows[k][row_len] (the opened rows behind the leaf digests)."""


def _witness_sets(lib, handle, n):
    """the trees of every item of an mh_witness_set as Python objects; frees the set"""
    def take(p, shape):
        size = int(np.prod(shape))
        return np.ctypeslib.as_array(p, shape=(size,)).reshape(shape).copy() if size else np.zeros(shape, dtype=np.uint64)
    lib.mh_witness_set_trees.restype = C.c_size_t
    lib.mh_witness_set_trees.argtypes = [C.c_void_p, C.c_size_t]
    lib.mh_witness_set_tree.argtypes = [C.c_void_p, C.c_size_t, C.c_size_t, C.POINTER(WitnessTreeView)]
    lib.mh_witness_set_free.argtypes = [C.c_void_p]
    lib.mh_witness_set_free.restype = None
    try:
        out = []
        for i in range(n):
            trees = []
            for t in range(lib.mh_witness_set_trees(handle, i)):
                v = WitnessTreeView()
                if lib.mh_witness_set_tree(handle, i, t, C.byref(v)) != 0:
                    raise MidenHipError("mh_witness_set_tree failed")
                w = WitnessTree(take(v.indices, (v.n_leaves,)), take(v.leaf_digests, (v.n_leaves, 4)), take(v.paths, (v.n_leaves, v.depth, 4)),
                                take(v.nodes, (v.n_nodes, 4)))
                w.kind, w.which, w.tree_root = int(v.kind), int(v.which), np.array(list(v.root), dtype=np.uint64)
                w.rows = take(v.rows, (v.n_leaves, v.row_len))
                trees.append(w)
            out.append(trees)
        return out
    finally:
        lib.mh_witness_set_free(handle)


class VerifyItem(C.Structure):
    _fields_ = [("log_trace_heights", C.POINTER(C.c_uint8)), ("public_values", u64p), ("n_public_values", C.c_size_t),
                ("pre_observe", u64p), ("n_pre_observe", C.c_size_t), ("fields", u64p), ("n_fields", C.c_size_t),
                ("commitments", u64p), ("n_commitments", C.c_size_t), ("preprocessed_root", u64p), ("external_user", C.c_void_p)]


class VerifyResult(C.Structure):
    _fields_ = [("code", C.c_int), ("digest", C.c_uint64 * 4), ("reason", C.c_char * 216)]


def _results(res, n):
    return [(True, np.array(list(res[i].digest), dtype=np.uint64)) if res[i].code == 0 else (False, res[i].reason.decode()) for i in range(n)]


def verify_batch(ctx, airs, items, params, challenger_state, external=None, lmcs="poseidon2", salt_elems=0, witness=False):
    """mh_verify_batch: many proofs of one statement shape -- host replay per item, every LMCS opening of the batch hashed on the
    device.  items = dicts with log_trace_heights, public_values, pre_observe, fields, commitments and optionally
    preprocessed_root; external as in verify().  Returns per item what verify() returns: (True, digest) or (False, reason).
    witness=True (mh_verify_batch_witness): returns (that list, per item the list of its WitnessTree -- one per opening of an accepted
    proof in proof order, [] for a rejected one)."""
    lib = ctx.lib
    n = len(airs)
    blobs = [_arr(a.blob) for a in airs]
    bp = (u64p * n)(*[_ptr(b) for b in blobs])
    bl = (C.c_size_t * n)(*[b.size for b in blobs])
    p = params if isinstance(params, PcsParams) else PcsParams.from_dict(params)
    st = _arr(challenger_state)
    if external in ("precompile_session", "precompile_session_ec_only"):
        external = C.cast(lib.mh_external_precompile_session_ec_only if external.endswith("ec_only") else lib.mh_external_precompile_session, EXTERNAL_FN)
    elif external == "logup_balance":
        external = C.cast(lib.mh_external_logup_balance, EXTERNAL_FN)
    arr = (VerifyItem * max(1, len(items)))()
    keep = []
    for k, it in enumerate(items):
        lh = (C.c_uint8 * n)(*[int(x) for x in it["log_trace_heights"]])
        pub, pre = _arr(list(it.get("public_values", ())) or [0]), _arr(list(it.get("pre_observe", ())) or [0])
        f, c = _arr(it["fields"]), _arr(np.asarray(it["commitments"], dtype=np.uint64).reshape(-1))
        proot = _arr(it["preprocessed_root"]) if it.get("preprocessed_root") is not None else None
        keep.append((lh, pub, pre, f, c, proot))
        arr[k].log_trace_heights = lh
        arr[k].public_values, arr[k].n_public_values = _ptr(pub), len(it.get("public_values", ()))
        arr[k].pre_observe, arr[k].n_pre_observe = _ptr(pre), len(it.get("pre_observe", ()))
        arr[k].fields, arr[k].n_fields = (_ptr(f) if f.size else None), f.size
        arr[k].commitments, arr[k].n_commitments = (_ptr(c) if c.size else None), c.size // 4
        arr[k].preprocessed_root = _ptr(proot) if proot is not None else None
        arr[k].external_user = None
    res = (VerifyResult * max(1, len(items)))()
    lib.mh_verify_batch.argtypes = [C.c_void_p, C.c_int, C.c_int, C.POINTER(PcsParams), C.c_int, C.POINTER(u64p), C.POINTER(C.c_size_t), u64p,
                                    EXTERNAL_FN, C.c_size_t, C.POINTER(VerifyItem), C.POINTER(VerifyResult)]
    ext = external if external is not None else C.cast(None, EXTERNAL_FN)
    if witness:
        handle = C.c_void_p()
        lib.mh_verify_batch_witness.argtypes = lib.mh_verify_batch.argtypes + [C.POINTER(C.c_void_p)]
        ctx.check(lib.mh_verify_batch_witness(ctx.h, Ctx.LMCS[lmcs], int(salt_elems), C.byref(p), n, bp, bl, _ptr(st), ext, len(items), arr, res,
                                              C.byref(handle)))
        return _results(res, len(items)), _witness_sets(lib, handle, len(items))
    ctx.check(lib.mh_verify_batch(ctx.h, Ctx.LMCS[lmcs], int(salt_elems), C.byref(p), n, bp, bl, _ptr(st), ext, len(items), arr, res))
    return _results(res, len(items))


# ---- the Miden VM statement in the library (csrc/miden.cpp): prove_stark's own shape, prover/src/lib.rs:317-355 ---------------------
class Miden:
    """mh_miden_load: the three AIRs of `MidenMultiAir` with their lookup programs on a context.  prove(core, chiplets, poseidon2,
    public_values[32], aux_inputs) -> Proof: host row-major matrices (mh_prove_miden) or Trace objects (mh_prove_miden_traces)."""

    def __init__(self, ctx):
        self.ctx = ctx
        h = C.c_void_p()
        ctx.check(ctx.lib.mh_miden_load(ctx.h, C.byref(h)))
        self.h = h
        ctx._children.add(self)

    def prove(self, core, chiplets, poseidon2, public_values, aux_inputs, hash_fn="poseidon2"):
        lib, mats = self.ctx.lib, (core, chiplets, poseidon2)
        pv, aux = _arr([int(x) for x in public_values]), _arr([int(x) for x in aux_inputs])
        assert pv.size == 32
        out = C.c_void_p()
        if all(isinstance(m, Trace) for m in mats):
            tr = (C.c_void_p * 3)(*[m.h for m in mats])
            rc = lib.mh_prove_miden_traces(self.ctx.h, self.h, C.c_int(Ctx.LMCS[hash_fn]), tr, _ptr(pv), _ptr(aux), C.c_size_t(aux.size), C.byref(out))
        else:
            hs = [np.ascontiguousarray(m, dtype=np.uint64) for m in mats]
            lg = [int(m.shape[0]).bit_length() - 1 for m in hs]
            assert [m.shape[1] for m in hs] == [51, 22, 16] and all(m.shape[0] == 1 << l for m, l in zip(hs, lg))
            rc = lib.mh_prove_miden(self.ctx.h, self.h, C.c_int(Ctx.LMCS[hash_fn]), _ptr(hs[0]), C.c_int(lg[0]), _ptr(hs[1]), C.c_int(lg[1]),
                                    _ptr(hs[2]), C.c_int(lg[2]), _ptr(pv), _ptr(aux), C.c_size_t(aux.size), C.byref(out))
        self.ctx.check(rc)
        return Proof(lib, out)

    def check(self, core, chiplets, poseidon2, public_values, aux_inputs, exact=False):
        """mh_check_miden(_traces): ExecutionTrace::check_constraints of this statement -> [CheckEntry] ([] when every constraint and the
        bus balance hold); host row-major matrices or Trace objects.  An unsatisfied statement is a result, not an error."""
        lib, mats = self.ctx.lib, (core, chiplets, poseidon2)
        pv, aux = _arr([int(x) for x in public_values]), _arr([int(x) for x in aux_inputs] or [0])
        flags = C.c_int(MH_CHECK_EXACT if exact else 0)
        if all(isinstance(m, Trace) for m in mats):
            tr = (C.c_void_p * 3)(*[m.h for m in mats])
            call = lambda out, cap, n: lib.mh_check_miden_traces(self.ctx.h, self.h, tr, _ptr(pv), _ptr(aux), C.c_size_t(len(aux_inputs)),
                                                                 flags, out, cap, n)
        else:
            hs = [np.ascontiguousarray(m, dtype=np.uint64) for m in mats]
            lg = [int(m.shape[0]).bit_length() - 1 for m in hs]
            if [m.shape[1] for m in hs] != [51, 22, 16] or any(m.shape[0] != 1 << l for m, l in zip(hs, lg)):
                raise MidenHipError("Miden.check: widths 51 / 22 / 16 and power-of-two heights expected")
            call = lambda out, cap, n: lib.mh_check_miden(self.ctx.h, self.h, _ptr(hs[0]), C.c_int(lg[0]), _ptr(hs[1]), C.c_int(lg[1]),
                                                          _ptr(hs[2]), C.c_int(lg[2]), _ptr(pv), _ptr(aux), C.c_size_t(len(aux_inputs)),
                                                          flags, out, cap, n)
        return _run_check(self.ctx, call)

    def check_balance(self, core, chiplets, poseidon2, public_values, aux_inputs, exact=False):
        """mh_check_balance_miden(_traces): the unmatched bus messages of this statement under check()'s challenges -> [BalanceEntry]
        ([] when the buses balance); host row-major matrices or Trace objects."""
        lib, mats = self.ctx.lib, (core, chiplets, poseidon2)
        pv, aux = _arr([int(x) for x in public_values]), _arr([int(x) for x in aux_inputs] or [0])
        flags = C.c_int(MH_CHECK_EXACT if exact else 0)
        if all(isinstance(m, Trace) for m in mats):
            tr = (C.c_void_p * 3)(*[m.h for m in mats])
            call = lambda *out: lib.mh_check_balance_miden_traces(self.ctx.h, self.h, tr, _ptr(pv), _ptr(aux), C.c_size_t(len(aux_inputs)),
                                                                  flags, *out)
        else:
            hs = [np.ascontiguousarray(m, dtype=np.uint64) for m in mats]
            lg = [int(m.shape[0]).bit_length() - 1 for m in hs]
            if [m.shape[1] for m in hs] != [51, 22, 16] or any(m.shape[0] != 1 << l for m, l in zip(hs, lg)):
                raise MidenHipError("Miden.check_balance: widths 51 / 22 / 16 and power-of-two heights expected")
            call = lambda *out: lib.mh_check_balance_miden(self.ctx.h, self.h, _ptr(hs[0]), C.c_int(lg[0]), _ptr(hs[1]), C.c_int(lg[1]),
                                                           _ptr(hs[2]), C.c_int(lg[2]), _ptr(pv), _ptr(aux), C.c_size_t(len(aux_inputs)),
                                                           flags, *out)
        return _run_balance(self.ctx, call)

    def fill_multiplicities(self, traces, public_values, aux_inputs, slots):
        """mh_fill_multiplicities_miden_traces: fill the multiplicity cells `slots` name ([(instance, lookup_column, fraction,
        main_column)], instance 0 / 1 / 2 = core / chiplets / poseidon2) in the three Trace objects, in place, under check()'s challenges
        and boundary pushes -> (cells written, [BalanceEntry])."""
        lib = self.ctx.lib
        if len(traces) != 3 or not all(isinstance(t, Trace) for t in traces):
            raise MidenHipError("Miden.fill_multiplicities: three Trace objects expected")
        pv, aux = _arr([int(x) for x in public_values]), _arr([int(x) for x in aux_inputs] or [0])
        tr = (C.c_void_p * 3)(*[t.h for t in traces])
        sa, ns = _slot_array(slots)
        call = lambda written, *out: lib.mh_fill_multiplicities_miden_traces(self.ctx.h, self.h, tr, _ptr(pv), _ptr(aux),
                                                                             C.c_size_t(len(aux_inputs)), sa, ns, written, *out)
        return _run_fill(self.ctx, call)

    def fill_range_table(self, traces, public_values, aux_inputs):
        """mh_fill_range_table_miden_traces: lay the range-check table (core columns RANGE_V and RANGE_M, core_air.RANGE_TABLE_SLOT) in
        the core Trace from the lookups of the three Trace objects, in place, under check()'s challenges and boundary pushes; whatever
        the two columns held is overwritten -> ([BalanceEntry], RangeTableInfo).  A table that does not fit the core trace raises
        MidenHipError; `e.info` says how many rows it needs."""
        lib = self.ctx.lib
        if len(traces) != 3 or not all(isinstance(t, Trace) for t in traces):
            raise MidenHipError("Miden.fill_range_table: three Trace objects expected")
        pv, aux = _arr([int(x) for x in public_values]), _arr([int(x) for x in aux_inputs] or [0])
        tr = (C.c_void_p * 3)(*[t.h for t in traces])
        info = RangeTableInfo()
        call = lambda written, *out: lib.mh_fill_range_table_miden_traces(self.ctx.h, self.h, tr, _ptr(pv), _ptr(aux),
                                                                          C.c_size_t(len(aux_inputs)), C.byref(info), written, *out)
        return _run_range(self.ctx, call, info)

    def poseidon2_trace(self, chiplets, log_n=None):
        """mh_miden_poseidon2_trace: the statement's third main trace derived on the device from the hasher controller's input rows of
        the device-resident chiplets Trace -> (Trace [2^log_n, 16], P2TraceInfo); log_n None: the smallest height.  A defect of the
        chiplets trace (a skipped perm_id, two states under one id, an id out of range, a log_n too small) raises MidenHipError with the
        library's message; `e.info` is the P2TraceInfo naming kind and row."""
        lib = self.ctx.lib
        if not isinstance(chiplets, Trace):
            raise MidenHipError("Miden.poseidon2_trace: a Trace object expected")
        lib.mh_miden_poseidon2_trace.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_void_p), C.POINTER(P2TraceInfo)]
        h, info = C.c_void_p(), P2TraceInfo()
        rc = lib.mh_miden_poseidon2_trace(self.ctx.h, chiplets.h, -1 if log_n is None else int(log_n), C.byref(h), C.byref(info))
        if rc != 0:
            e = MidenHipError(f"libmidenhip error {rc}: {lib.mh_last_error(self.ctx.h).decode()}")
            e.info = info
            raise e
        return Trace.from_handle(self.ctx, h, int(info.log_n), 16), info

    def memory_section(self, chiplets, start_row, accesses, want_rows=False):
        """mh_miden_memory_section: the memory chiplet's rows written in place into the device-resident chiplets Trace at rows
        [start_row, start_row + n) from the access list (MEM_ACCESS_DTYPE records in program order): columns 0..2 = 1, 1, 0 and
        columns 3..19; columns 20, 21 and every other row stay -> (MemSectionInfo, row_of or None).  A defect of the list, or a section
        that does not fit, raises MidenHipError with `e.info`; nothing was written then."""
        lib = self.ctx.lib
        if not isinstance(chiplets, Trace):
            raise MidenHipError("Miden.memory_section: a Trace object expected")
        acc, ap = _mem_accesses(accesses)
        lib.mh_miden_memory_section.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_size_t, C.c_void_p, C.POINTER(MemSectionInfo)]
        info = MemSectionInfo()
        rows = np.zeros(acc.size, dtype=np.uint32) if want_rows else None
        rp = rows.ctypes.data_as(C.c_void_p) if want_rows and acc.size else None
        rc = lib.mh_miden_memory_section(self.ctx.h, chiplets.h, int(start_row), ap, acc.size, rp, C.byref(info))
        _mem_section_result(lib, self.ctx, rc, info)
        return info, rows

    def hasher_section(self, chiplets, ops, felts, want_results=False):
        """mh_miden_hasher_section: the hasher controller's rows written in place into rows [0, n_rows) of the device-resident chiplets
        Trace from the op list (HASH_OP_DTYPE records in program order, operands in `felts`): column 0 = 0 and columns 1..20; column 21
        and every row from n_rows on stay -> (HasherSectionInfo, results or None).  A defect of the list, or a section that does not
        fit, raises MidenHipError with `e.info`; nothing was written then."""
        lib = self.ctx.lib
        if not isinstance(chiplets, Trace):
            raise MidenHipError("Miden.hasher_section: a Trace object expected")
        o, op, f, fp = _hash_ops(ops, felts)
        lib.mh_miden_hasher_section.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p,
                                                C.POINTER(HasherSectionInfo)]
        info = HasherSectionInfo()
        res = np.zeros(o.size, dtype=HASH_RESULT_DTYPE) if want_results else None
        rp = res.ctypes.data_as(C.c_void_p) if want_results and o.size else None
        rc = lib.mh_miden_hasher_section(self.ctx.h, chiplets.h, op, o.size, fp, f.size, rp, C.byref(info))
        _mem_section_result(lib, self.ctx, rc, info)
        return info, res

    def bitwise_section(self, chiplets, start_row, ops, want_results=False):
        """mh_miden_bitwise_section: the bitwise chiplet's rows written in place into the device-resident chiplets Trace at rows
        [start_row, start_row + 8 n_ops): columns 0, 1 = 1, 0 and columns 2..14; everything else stays -> (BitwiseSectionInfo, results
        or None).  A defect of the list, or a section that does not fit, raises MidenHipError with `e.info`; nothing was written then."""
        lib = self.ctx.lib
        if not isinstance(chiplets, Trace):
            raise MidenHipError("Miden.bitwise_section: a Trace object expected")
        o, op = _bitwise_ops(ops)
        lib.mh_miden_bitwise_section.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_size_t, C.c_void_p,
                                                 C.POINTER(BitwiseSectionInfo)]
        info = BitwiseSectionInfo()
        res = np.zeros(o.size, dtype=np.uint32) if want_results else None
        rp = res.ctypes.data_as(C.c_void_p) if want_results and o.size else None
        rc = lib.mh_miden_bitwise_section(self.ctx.h, chiplets.h, int(start_row), op, o.size, rp, C.byref(info))
        _mem_section_result(lib, self.ctx, rc, info)
        return info, res

    def ace_section(self, chiplets, start_row, evals, felts):
        """mh_miden_ace_section: the ACE chiplet's rows written in place into the device-resident chiplets Trace from start_row on:
        columns 0..3 = 1, 1, 1, 0 and columns 4..19; everything else stays -> AceSectionInfo.  A defect of the list, or a section that
        does not fit, raises MidenHipError with `e.info`; nothing was written then."""
        lib = self.ctx.lib
        if not isinstance(chiplets, Trace):
            raise MidenHipError("Miden.ace_section: a Trace object expected")
        e, ep, f, fp = _ace_evals(evals, felts)
        lib.mh_miden_ace_section.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t,
                                             C.POINTER(AceSectionInfo)]
        info = AceSectionInfo()
        rc = lib.mh_miden_ace_section(self.ctx.h, chiplets.h, int(start_row), ep, e.size, fp, f.size, C.byref(info))
        _mem_section_result(lib, self.ctx, rc, info)
        return info

    def kernel_rom_section(self, chiplets, start_row, procs, calls, want_digests=False):
        """mh_miden_kernel_rom_section: the kernel ROM's rows written in place into the device-resident chiplets Trace from start_row
        on: columns 0..4 = 1, 1, 1, 1, 0 and columns 5..9; everything else stays -> (KernelRomSectionInfo, digests or None).  A defect,
        or a section that does not fit, raises MidenHipError with `e.info`; nothing was written then."""
        lib = self.ctx.lib
        if not isinstance(chiplets, Trace):
            raise MidenHipError("Miden.kernel_rom_section: a Trace object expected")
        p, pp = _digests(procs)
        k, kp = _digests(calls)
        lib.mh_miden_kernel_rom_section.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t,
                                                    C.c_void_p, C.POINTER(KernelRomSectionInfo)]
        info = KernelRomSectionInfo()
        dig = np.zeros((p.shape[0], 4), dtype=np.uint64) if want_digests else None
        dp = dig.ctypes.data_as(C.c_void_p) if want_digests and dig.size else None
        rc = lib.mh_miden_kernel_rom_section(self.ctx.h, chiplets.h, int(start_row), pp, p.shape[0], kp, k.shape[0], dp, C.byref(info))
        _mem_section_result(lib, self.ctx, rc, info)
        return info, (dig[:int(info.n_rows)] if want_digests else None)

    def chiplets_frame(self, chiplets, padding_start):
        """mh_miden_chiplets_frame: chip_clk = row + 1 in column 21 of every row of the device-resident chiplets Trace and, from
        padding_start on, ones in columns 0..4 and zeros in columns 5..20; nothing else is touched."""
        lib = self.ctx.lib
        if not isinstance(chiplets, Trace):
            raise MidenHipError("Miden.chiplets_frame: a Trace object expected")
        lib.mh_miden_chiplets_frame.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64]
        self.ctx.check(lib.mh_miden_chiplets_frame(self.ctx.h, chiplets.h, int(padding_start)))

    def chiplets_build(self, lists, log_n=None):
        """mh_miden_chiplets_build: the finished chiplets trace on the device from the five lists of one executed program -> (Trace
        [2^log_n, 22], ChipletsInfo); log_n None: max(6, ceil log2 trace_len).  `lists` is a mapping with the keys hash_ops, hash_felts
        (HASH_OP_DTYPE, uint64), bitwise_ops (BITWISE_OP_DTYPE), mem_accesses (MEM_ACCESS_DTYPE), ace_evals, ace_felts (ACE_EVAL_DTYPE,
        uint64), kernel_procs, kernel_calls (uint64 [n][4]); a missing key is an empty list.  A defect of a list, or a trace that does
        not fit, raises MidenHipError with `e.info` naming the section; no trace exists then."""
        lib = self.ctx.lib
        ho, hop, hf, hfp = _hash_ops(_records(lists.get("hash_ops", ()), HASH_OP_DTYPE), lists.get("hash_felts", ()))
        bo, bop = _bitwise_ops(lists.get("bitwise_ops", ()))
        ma, map_ = _mem_accesses(_records(lists.get("mem_accesses", ()), MEM_ACCESS_DTYPE))
        ae, aep, af, afp = _ace_evals(lists.get("ace_evals", ()), lists.get("ace_felts", ()))
        kp, kpp = _digests(lists.get("kernel_procs", ()))
        kc, kcp = _digests(lists.get("kernel_calls", ()))
        ls = ChipletsLists(hop, ho.size, hfp, hf.size, bop, bo.size, map_, ma.size, aep, ae.size, afp, af.size, kpp, kp.shape[0], kcp, kc.shape[0])
        lib.mh_miden_chiplets_build.argtypes = [C.c_void_p, C.POINTER(ChipletsLists), C.c_int, C.POINTER(C.c_void_p), C.POINTER(ChipletsInfo)]
        h, info = C.c_void_p(), ChipletsInfo()
        rc = lib.mh_miden_chiplets_build(self.ctx.h, C.byref(ls), -1 if log_n is None else int(log_n), C.byref(h), C.byref(info))
        if rc != 0:
            assert not h.value
        _mem_section_result(lib, self.ctx, rc, info)
        return Trace.from_handle(self.ctx, h, int(info.log_n), 22), info

    def free(self):
        if getattr(self, "h", None) and self.ctx.h:
            self.ctx.lib.mh_miden_free(self.h)
        self.h = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def verify_miden(public_values, aux_inputs, proof_bytes, hash_fn="poseidon2"):
    """mh_verify_miden (host only): StarkProofData bytes of a Miden proof -> (True, digest) or (False, reason)."""
    lib = load_library()
    pv, aux = _arr([int(x) for x in public_values]), _arr([int(x) for x in aux_inputs] or [0])
    buf = (C.c_uint8 * max(1, len(proof_bytes))).from_buffer_copy(bytes(proof_bytes) or b"\0")
    digest, err = np.zeros(4, dtype=np.uint64), C.create_string_buffer(512)
    lib.mh_verify_miden.argtypes = [C.c_int, u64p, u64p, C.c_size_t, C.c_void_p, C.c_size_t, u64p, C.c_char_p, C.c_size_t]
    rc = lib.mh_verify_miden(Ctx.LMCS[hash_fn], _ptr(pv), _ptr(aux), len(aux_inputs), buf, len(proof_bytes), _ptr(digest), err, 512)
    return (True, digest) if rc == 0 else (False, err.value.decode())


class MidenVerifyItem(C.Structure):
    _fields_ = [("public_values", u64p), ("aux_inputs", u64p), ("n_aux_inputs", C.c_size_t), ("proof_bytes", C.c_void_p), ("n_bytes", C.c_size_t)]


def verify_miden_batch(ctx, items, hash_fn="poseidon2", witness=False):
    """mh_verify_miden_batch: items = (public_values, aux_inputs, proof_bytes) per proof; per item what verify_miden returns.
    witness=True (mh_verify_miden_batch_witness): (that list, per item its WitnessTree list) as verify_batch(witness=True)."""
    n = len(items)
    arr = (MidenVerifyItem * max(1, n))()
    keep = []
    for k, (public_values, aux_inputs, proof_bytes) in enumerate(items):
        pv, aux = _arr([int(x) for x in public_values]), _arr([int(x) for x in aux_inputs] or [0])
        buf = (C.c_uint8 * max(1, len(proof_bytes))).from_buffer_copy(bytes(proof_bytes) or b"\0")
        keep.append((pv, aux, buf))
        arr[k].public_values, arr[k].aux_inputs, arr[k].n_aux_inputs = _ptr(pv), _ptr(aux), len(aux_inputs)
        arr[k].proof_bytes, arr[k].n_bytes = C.cast(buf, C.c_void_p), len(proof_bytes)
    res = (VerifyResult * max(1, n))()
    if witness:
        handle = C.c_void_p()
        ctx.lib.mh_verify_miden_batch_witness.argtypes = [C.c_void_p, C.c_int, C.c_size_t, C.POINTER(MidenVerifyItem), C.POINTER(VerifyResult),
                                                          C.POINTER(C.c_void_p)]
        ctx.check(ctx.lib.mh_verify_miden_batch_witness(ctx.h, Ctx.LMCS[hash_fn], n, arr, res, C.byref(handle)))
        return _results(res, n), _witness_sets(ctx.lib, handle, n)
    ctx.lib.mh_verify_miden_batch.argtypes = [C.c_void_p, C.c_int, C.c_size_t, C.POINTER(MidenVerifyItem), C.POINTER(VerifyResult)]
    ctx.check(ctx.lib.mh_verify_miden_batch(ctx.h, Ctx.LMCS[hash_fn], n, arr, res))
    return _results(res, n)


class Precompile:
    """mh_precompile_load: the twelve AIRs of `ChipletAir::all()` with their lookup programs on a context, the byte-pair table uploaded
    (its commitment is made per hash function on first use and kept: session/preprocessed_cache.rs).
    prove(mains[12], public_root[4]) -> Proof: host row-major matrices (mh_prove_precompile) or Trace objects (mh_prove_precompile_traces)
    -- `SessionTraces::prove_stark`'s shape (precompiles-prover/src/session/prove.rs:295-330)."""
    WIDTHS = (42, 32, 68, 3, 67, 39, 44, 30, 6, 14, 21, 38)

    def __init__(self, ctx):
        self.ctx = ctx
        h = C.c_void_p()
        ctx.check(ctx.lib.mh_precompile_load(ctx.h, C.byref(h)))
        self.h = h
        ctx._children.add(self)

    def preprocessed_root(self, hash_fn="poseidon2"):
        root = np.zeros(4, dtype=np.uint64)
        self.ctx.check(self.ctx.lib.mh_precompile_preprocessed_root(self.h, C.c_int(Ctx.LMCS[hash_fn]), _ptr(root)))
        return root

    def prove(self, mains, public_root, hash_fn="poseidon2"):
        lib = self.ctx.lib
        assert len(mains) == 12
        root = _arr([int(x) for x in public_root])
        assert root.size == 4
        out = C.c_void_p()
        if all(isinstance(m, Trace) for m in mains):
            tr = (C.c_void_p * 12)(*[m.h for m in mains])
            rc = lib.mh_prove_precompile_traces(self.ctx.h, self.h, C.c_int(Ctx.LMCS[hash_fn]), tr, _ptr(root), C.byref(out))
        else:
            hs = [np.ascontiguousarray(m, dtype=np.uint64) for m in mains]
            lg = [int(m.shape[0]).bit_length() - 1 for m in hs]
            assert tuple(m.shape[1] for m in hs) == self.WIDTHS and all(m.shape[0] == 1 << l for m, l in zip(hs, lg))
            ptrs = (u64p * 12)(*[_ptr(m) for m in hs])
            rc = lib.mh_prove_precompile(self.ctx.h, self.h, C.c_int(Ctx.LMCS[hash_fn]), ptrs, (C.c_int * 12)(*lg), _ptr(root), C.byref(out))
        self.ctx.check(rc)
        return Proof(lib, out)

    def check(self, mains, public_root, exact=False):
        """mh_check_precompile(_traces): SessionTraces::check -> [CheckEntry] ([] when the session is satisfied)."""
        lib = self.ctx.lib
        if len(mains) != 12:
            raise MidenHipError("Precompile.check: twelve main traces expected")
        root = _arr([int(x) for x in public_root])
        flags = C.c_int(MH_CHECK_EXACT if exact else 0)
        if all(isinstance(m, Trace) for m in mains):
            tr = (C.c_void_p * 12)(*[m.h for m in mains])
            call = lambda out, cap, n: lib.mh_check_precompile_traces(self.ctx.h, self.h, tr, _ptr(root), flags, out, cap, n)
        else:
            hs = [np.ascontiguousarray(m, dtype=np.uint64) for m in mains]
            lg = [int(m.shape[0]).bit_length() - 1 for m in hs]
            if tuple(m.shape[1] for m in hs) != self.WIDTHS or any(m.shape[0] != 1 << l for m, l in zip(hs, lg)):
                raise MidenHipError("Precompile.check: the AIRs' widths and power-of-two heights expected")
            ptrs = (u64p * 12)(*[_ptr(m) for m in hs])
            lh = (C.c_int * 12)(*lg)
            call = lambda out, cap, n: lib.mh_check_precompile(self.ctx.h, self.h, ptrs, lh, _ptr(root), flags, out, cap, n)
        return _run_check(self.ctx, call)

    def check_balance(self, mains, public_root, exact=False):
        """mh_check_balance_precompile(_traces): the unmatched bus messages of the session under check()'s challenges -> [BalanceEntry]
        ([] when the buses balance)."""
        lib = self.ctx.lib
        if len(mains) != 12:
            raise MidenHipError("Precompile.check_balance: twelve main traces expected")
        root = _arr([int(x) for x in public_root])
        flags = C.c_int(MH_CHECK_EXACT if exact else 0)
        if all(isinstance(m, Trace) for m in mains):
            tr = (C.c_void_p * 12)(*[m.h for m in mains])
            call = lambda *out: lib.mh_check_balance_precompile_traces(self.ctx.h, self.h, tr, _ptr(root), flags, *out)
        else:
            hs = [np.ascontiguousarray(m, dtype=np.uint64) for m in mains]
            lg = [int(m.shape[0]).bit_length() - 1 for m in hs]
            if tuple(m.shape[1] for m in hs) != self.WIDTHS or any(m.shape[0] != 1 << l for m, l in zip(hs, lg)):
                raise MidenHipError("Precompile.check_balance: the AIRs' widths and power-of-two heights expected")
            ptrs = (u64p * 12)(*[_ptr(m) for m in hs])
            lh = (C.c_int * 12)(*lg)
            call = lambda *out: lib.mh_check_balance_precompile(self.ctx.h, self.h, ptrs, lh, _ptr(root), flags, *out)
        return _run_balance(self.ctx, call)

    def fill_multiplicities(self, traces, public_root, slots):
        """mh_fill_multiplicities_precompile_traces: fill the multiplicity cells `slots` name ([(instance, lookup_column, fraction,
        main_column)], instance = chiplet index) in the twelve Trace objects, in place, under check()'s challenges and the verifier's
        fixed consumes -> (cells written, [BalanceEntry])."""
        lib = self.ctx.lib
        if len(traces) != 12 or not all(isinstance(t, Trace) for t in traces):
            raise MidenHipError("Precompile.fill_multiplicities: twelve Trace objects expected")
        root = _arr([int(x) for x in public_root])
        tr = (C.c_void_p * 12)(*[t.h for t in traces])
        sa, ns = _slot_array(slots)
        call = lambda written, *out: lib.mh_fill_multiplicities_precompile_traces(self.ctx.h, self.h, tr, _ptr(root), sa, ns, written, *out)
        return _run_fill(self.ctx, call)

    def poseidon2_trace(self, absorptions, blocks, refs=None, log_n=None, want_digests=False, want_outputs=False):
        """poseidon2_chiplet_trace on this object's context: the session's trace 1 (Poseidon2) from the absorption ledger."""
        return poseidon2_chiplet_trace(self.ctx, absorptions, blocks, refs, log_n, want_digests, want_outputs)

    def uint_traces(self, rows, muls, adds, log_usm=None, log_add=None):
        """uint_traces on this object's context: the session's traces 6 (UintStoreMul) and 7 (UintAdd) from the uint ledgers."""
        return uint_traces(self.ctx, rows, muls, adds, log_usm, log_add)

    def ec_traces(self, groups, points, adds, exprs, terms, log_groups=-1, log_points=-1, log_add=-1, log_msm=-1):
        """ec_traces on this object's context: the session's traces 8..11 (EcGroups, EcPointStore, EcGroupAdd, EcMsm) from the EC ledgers."""
        return ec_traces(self.ctx, groups, points, adds, exprs, terms, log_groups, log_points, log_add, log_msm)

    def chunk_node_trace(self, p2, data, digests, records, log_n=-1):
        """chunk_node_trace on this object's context: the session's trace 0 (ChunkNode) from the node records and the Poseidon2 Trace."""
        return chunk_node_trace(self.ctx, p2, data, digests, records, log_n)

    def transcript_eval_trace(self, p2, nodes, terms, limbs, root, log_n=-1, want_root=True):
        """transcript_eval_trace on this object's context: the session's trace 5 (TranscriptEval) from the transcript's nodes and the
        Poseidon2 Trace."""
        return transcript_eval_trace(self.ctx, p2, nodes, terms, limbs, root, log_n, want_root)

    def keccak_traces(self, messages, chunk_heads, log_round=None, log_sponge=None, want_digests=False):
        """keccak_traces on this object's context: the session's traces 2 (Keccak round) and 4 (Keccak sponge) from the messages."""
        return keccak_traces(self.ctx, messages, chunk_heads, log_round, log_sponge, want_digests)

    def free(self):
        if getattr(self, "h", None) and self.ctx.h:
            self.ctx.lib.mh_precompile_free(self.h)
        self.h = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def precompile_setup_root(hash_fn="poseidon2"):
    """mh_precompile_setup_root (host only): the byte-pair table's setup commitment under `hash_fn`, derived from the table on the CPU
    (once per hash function and process) -- equal to Precompile.preprocessed_root(hash_fn) of a prover's context."""
    lib = load_library()
    root = np.zeros(4, dtype=np.uint64)
    lib.mh_precompile_setup_root.argtypes = [C.c_int, u64p]
    rc = lib.mh_precompile_setup_root(Ctx.LMCS[hash_fn], _ptr(root))
    if rc != 0:
        raise MidenHipError(f"mh_precompile_setup_root failed ({rc})")
    return root


def verify_precompile(preprocessed_root, public_root, proof_bytes, hash_fn="poseidon2"):
    """mh_verify_precompile (host only): StarkProofData bytes of a precompile-session proof -> (True, digest) or (False, reason).
    preprocessed_root=None (the verifier's normal call): the setup commitment is derived from the byte-pair table; a root that is given
    is checked against the derived one before the proof is read."""
    lib = load_library()
    pr = None if preprocessed_root is None else _arr([int(x) for x in preprocessed_root])
    root = _arr([int(x) for x in public_root])
    buf = (C.c_uint8 * max(1, len(proof_bytes))).from_buffer_copy(bytes(proof_bytes) or b"\0")
    digest, err = np.zeros(4, dtype=np.uint64), C.create_string_buffer(512)
    lib.mh_verify_precompile.argtypes = [C.c_int, u64p, u64p, C.c_void_p, C.c_size_t, u64p, C.c_char_p, C.c_size_t]
    rc = lib.mh_verify_precompile(Ctx.LMCS[hash_fn], None if pr is None else _ptr(pr), _ptr(root), buf, len(proof_bytes), _ptr(digest), err, 512)
    return (True, digest) if rc == 0 else (False, err.value.decode())


def precompile_pre_observe(params, preprocessed_root, public_root):
    """mh_precompile_pre_observe: observe_protocol_params | preprocessed commitment | the default statement framing (19 felts)."""
    lib = load_library()
    p = params if isinstance(params, PcsParams) else PcsParams.from_dict(params)
    pr, root, out = _arr([int(x) for x in preprocessed_root]), _arr([int(x) for x in public_root]), np.zeros(19, dtype=np.uint64)
    if lib.mh_precompile_pre_observe(C.byref(p), _ptr(pr), _ptr(root), _ptr(out)) != 0:
        raise MidenHipError("mh_precompile_pre_observe failed")
    return [int(x) for x in out]


def precompile_air_blob(which, lookup=False):
    """mh_precompile_air_blob: the embedded constraint DAG (lookup=False) or lookup program of AIR `which` of `ChipletAir::all()`."""
    lib = load_library()
    w, n = u64p(), C.c_size_t(0)
    if lib.mh_precompile_air_blob(C.c_int(which), C.c_int(1 if lookup else 0), C.byref(w), C.byref(n)) != 0:
        raise MidenHipError("mh_precompile_air_blob: no such AIR")
    return np.ctypeslib.as_array(w, shape=(n.value,)).copy()


def miden_pre_observe(params, public_values, aux_inputs):
    """mh_miden_pre_observe: observe_protocol_params + `MidenMultiAir::observe` (56 felts)."""
    lib = load_library()
    p = params if isinstance(params, PcsParams) else PcsParams.from_dict(params)
    pv, aux, out = _arr([int(x) for x in public_values]), _arr([int(x) for x in aux_inputs] or [0]), np.zeros(56, dtype=np.uint64)
    rc = lib.mh_miden_pre_observe(C.byref(p), _ptr(pv), _ptr(aux), C.c_size_t(len(aux_inputs)), _ptr(out))
    if rc != 0:
        raise MidenHipError("mh_miden_pre_observe: malformed public values / aux inputs")
    return [int(x) for x in out]


def miden_hash_kernel_digests(kernel_felts):
    lib = load_library()
    k, out = _arr([int(x) for x in kernel_felts] or [0]), np.zeros(4, dtype=np.uint64)
    if lib.mh_miden_hash_kernel_digests(_ptr(k), C.c_size_t(len(kernel_felts)), _ptr(out)) != 0:
        raise MidenHipError("mh_miden_hash_kernel_digests: whole words, at most 255 procedures")
    return [int(x) for x in out]


def miden_eval_external(randomness, aux_inputs, aux_values):
    """mh_miden_eval_external: randomness [(a0, a1), (b0, b1)], aux_values = per AIR [(c0, c1)] -> the assertion (c0, c1), or None
    when the library refuses the shape / meets a zero denominator."""
    lib = load_library()
    rnd = _arr([int(x) for pair in randomness for x in pair])
    aux = _arr([int(x) for x in aux_inputs] or [0])
    vals = [_arr([int(x) for pair in v for x in pair] or [0]) for v in aux_values]
    vp = (u64p * len(vals))(*[_ptr(v) for v in vals])
    nv = (C.c_size_t * len(vals))(*[len(v) for v in aux_values])
    out = np.zeros(2, dtype=np.uint64)
    rc = lib.mh_miden_eval_external(_ptr(rnd), _ptr(aux), C.c_size_t(len(aux_inputs)), vp, nv, C.c_int(len(vals)), _ptr(out))
    return (int(out[0]), int(out[1])) if rc == 0 else None


def miden_constants():
    """(pcs params dict, challenger state) of the production configuration as the library holds them."""
    lib = load_library()
    p, st = PcsParams(), np.zeros(12, dtype=np.uint64)
    lib.mh_miden_pcs_params(C.byref(p))
    lib.mh_miden_challenger_state(_ptr(st))
    return {k: int(getattr(p, k)) for k, _ in PcsParams._fields_}, [int(x) for x in st]


def miden_air_blob(which):
    lib = load_library()
    w, n = u64p(), C.c_size_t()
    assert lib.mh_miden_air_blob(C.c_int(which), C.byref(w), C.byref(n)) == 0
    return np.ctypeslib.as_array(w, shape=(n.value,)).copy()


def jit_precompile(blob, cache_dir=None):
    """mh_jit_precompile (host only, no GPU): compile the chunk kernels of an AIR / lookup blob into the cache directory.
    -> number of chunk kernels."""
    lib = load_library()
    b = _arr(blob)
    k = C.c_int(0)
    old = os.environ.get("MH_JIT_CACHE_DIR")
    if cache_dir is not None:
        os.environ["MH_JIT_CACHE_DIR"] = cache_dir
    try:
        rc = lib.mh_jit_precompile(_ptr(b), C.c_size_t(b.size), C.byref(k))
    finally:
        if cache_dir is not None:
            if old is None:
                os.environ.pop("MH_JIT_CACHE_DIR", None)
            else:
                os.environ["MH_JIT_CACHE_DIR"] = old
    if rc != 0:
        raise MidenHipError(f"mh_jit_precompile failed: {rc}")
    return int(k.value)


def grind_bytes(ctx, input_bytes, bits):
    """mh_grind_bytes: device PoW search for a hash challenger whose input buffer holds `input_bytes` (Blake3 / Keccak context)."""
    data = bytes(input_bytes)
    w = C.c_uint64(0)
    ctx.check(ctx.lib.mh_grind_bytes(ctx.h, data, C.c_size_t(len(data)), C.c_int(bits), C.byref(w)))
    return int(w.value)


def blake3(data):
    """mh_blake3 (host only): the 32-byte BLAKE3 digest of `data`."""
    lib = load_library()
    data = bytes(data)
    out = C.create_string_buffer(32)
    lib.mh_blake3.restype = None
    lib.mh_blake3(data, C.c_size_t(len(data)), out)
    return out.raw
