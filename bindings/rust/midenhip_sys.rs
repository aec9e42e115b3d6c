//! Raw FFI declarations for libmidenhip (include/midenhip.h) — the `-sys` layer of the shim described in
//! INTEGRATION.md.  One declaration per exported symbol; no logic.  NOT COMPILED IN THIS REPOSITORY: the build image
//! has no Rust toolchain, so this file is written against the header by hand (tests/test_abi.py checks that the symbol
//! list here, the header and the shared library agree).  Link with `-lmidenhip`.
#![allow(non_camel_case_types)]
use core::ffi::{c_char, c_double, c_int, c_long, c_void};

macro_rules! opaque { ($($n:ident),*) => { $( #[repr(C)] pub struct $n { _p: [u8; 0] } )* } }
opaque!(mh_ctx, mh_trace, mh_tree, mh_air, mh_proof, mh_shard, mh_lookup, mh_session, mh_miden, mh_precompile, mh_pcs);

pub const MH_OK: c_int = 0;
pub const MH_ERR_INVALID: c_int = 1;
pub const MH_ERR_HIP: c_int = 2;
pub const MH_ERR_OOM: c_int = 3;
pub const MH_ERR_INTERNAL: c_int = 4;
pub const MH_ERR_COMM: c_int = 5;
/// mh_check_*: the trace does not satisfy the statement; the entries say where.
pub const MH_ERR_UNSATISFIED: c_int = 6;
/// mh_check_* flags: evaluate every constraint on every row (no fold screen).
pub const MH_CHECK_EXACT: c_int = 1;

/// One failing constraint (or external assertion, instance = -1) of a constraint check.
#[repr(C)]
#[derive(Clone, Copy, Debug, Default, PartialEq, Eq)]
pub struct mh_check_entry {
    pub instance: i32,
    pub constraint: u32,
    pub rows: u64,
    pub first_row: u64,
    pub value: [u64; 2],
}

/// mh_balance_entry.first_push: the push list was not collected (more than 2^22 pushes).
pub const MH_BALANCE_NO_PUSHES: u64 = u64::MAX;

/// mh_fill_multiplicities*: fraction `fraction` of LogUp column `lookup_column` of instance `instance` has a multiplicity that is
/// affine in main-trace column `main_column`.
#[repr(C)]
#[derive(Clone, Copy, Debug, Default, PartialEq, Eq)]
pub struct mh_mult_slot {
    pub instance: i32,
    pub lookup_column: u32,
    pub fraction: u32,
    pub main_column: u32,
}

/// mh_fill_range_table: fraction `fraction` of LogUp column `lookup_column` of instance `instance` is the range table's provider; its
/// denominator encodes main-trace column `value_column`, its multiplicity is affine in `mult_column`.
#[repr(C)]
#[derive(Clone, Copy, Debug, Default, PartialEq, Eq)]
pub struct mh_range_slot {
    pub instance: i32,
    pub lookup_column: u32,
    pub fraction: u32,
    pub value_column: u32,
    pub mult_column: u32,
}

/// mh_fill_range_table*: the table's size against the declaring trace's height (filled also when the table does not fit).
#[repr(C)]
#[derive(Clone, Copy, Debug, Default, PartialEq, Eq)]
pub struct mh_range_table_info {
    pub n_values: u64,
    pub rows_needed: u64,
    pub rows_available: u64,
}

/// mh_poseidon2_trace_build / mh_miden_poseidon2_trace: what was built, or the defect that refused the input (see midenhip.h).
#[repr(C)]
#[derive(Clone, Copy, Debug, Default, PartialEq, Eq)]
pub struct mh_p2_trace_info {
    pub n_requests: u64,
    pub n_input_rows: u64,
    pub log_n: i32,
    pub defect: i32,
    pub defect_row: u64,
}

/// One memory access of mh_memory_section_build / mh_miden_memory_section, in program order (48 bytes).  kind: bit 0 = read, bit 1 =
/// word access; addr is the element address; value: [0] for an element write, [0..3] for a word write, ignored by reads.
#[repr(C)]
#[derive(Clone, Copy, Debug, Default, PartialEq, Eq)]
pub struct mh_mem_access {
    pub ctx: u32,
    pub addr: u32,
    pub clk: u32,
    pub kind: u32,
    pub value: [u64; 4],
}

/// mh_memory_section_build / mh_miden_memory_section: what was written, or the defect that refused the list (see midenhip.h).
#[repr(C)]
#[derive(Clone, Copy, Debug, Default, PartialEq, Eq)]
pub struct mh_mem_section_info {
    pub n_rows: u64,
    pub n_words: u64,
    pub n_contexts: u64,
    pub log_n: i32,
    pub defect: i32,
    pub defect_index: u64,
}

/// One hash operation of mh_hasher_section_build / mh_miden_hasher_section, in program order (24 bytes).  kind: 0 permute, 1 control
/// block, 2 basic block, 3 merkle verify, 4 merkle update; count: batches or depth; index: node index or domain; payload: offset of the
/// operands in `felts`.
#[repr(C)]
#[derive(Clone, Copy, Debug, Default, PartialEq, Eq)]
pub struct mh_hash_op {
    pub kind: u32,
    pub count: u32,
    pub index: u64,
    pub payload: u64,
}

/// What one hash operation gave: the 1-based row of its first row, its last post-state, the old root of a merkle update.
#[repr(C)]
#[derive(Clone, Copy, Debug, Default, PartialEq, Eq)]
pub struct mh_hash_result {
    pub addr: u64,
    pub state: [u64; 12],
    pub old_root: [u64; 4],
}

/// mh_hasher_section_build / mh_miden_hasher_section: what was written, or the defect that refused the list (see midenhip.h).
#[repr(C)]
#[derive(Clone, Copy, Debug, Default, PartialEq, Eq)]
pub struct mh_hasher_section_info {
    pub n_rows: u64,
    pub n_permutations: u64,
    pub n_requests: u64,
    pub mrupdate_id: u64,
    pub log_n: i32,
    pub defect: i32,
    pub defect_index: u64,
}

/// One bitwise operation of mh_bitwise_section_build / mh_miden_bitwise_section, in program order (12 bytes).  op: 0 AND, 1 XOR.
#[repr(C)]
#[derive(Clone, Copy, Debug, Default, PartialEq, Eq)]
pub struct mh_bitwise_op {
    pub op: u32,
    pub a: u32,
    pub b: u32,
}

/// mh_bitwise_section_build / mh_miden_bitwise_section: what was written, or the defect that refused the list (see midenhip.h).
#[repr(C)]
#[derive(Clone, Copy, Debug, Default, PartialEq, Eq)]
pub struct mh_bitwise_section_info {
    pub n_rows: u64,
    pub log_n: i32,
    pub defect: i32,
    pub defect_index: u64,
}

/// One circuit evaluation of mh_ace_section_build / mh_miden_ace_section, in clock order (32 bytes).  payload: offset in `felts` of
/// 2 * num_vars felts (the words as read from memory) followed by num_eval instruction felts.
#[repr(C)]
#[derive(Clone, Copy, Debug, Default, PartialEq, Eq)]
pub struct mh_ace_eval {
    pub ctx: u32,
    pub ptr: u32,
    pub clk: u32,
    pub num_vars: u32,
    pub num_eval: u32,
    pub reserved: u32,
    pub payload: u64,
}

/// mh_ace_section_build / mh_miden_ace_section: what was written, or the defect that refused the list (see midenhip.h).
#[repr(C)]
#[derive(Clone, Copy, Debug, Default, PartialEq, Eq)]
pub struct mh_ace_section_info {
    pub n_rows: u64,
    pub n_wires: u64,
    pub n_gates: u64,
    pub n_rounds: u64,
    pub log_n: i32,
    pub defect: i32,
    pub defect_index: u64,
    pub defect_gate: u64,
}

/// mh_kernel_rom_section_build / mh_miden_kernel_rom_section: what was written, or the defect that refused the lists (see midenhip.h).
#[repr(C)]
#[derive(Clone, Copy, Debug, Default, PartialEq, Eq)]
pub struct mh_kernel_rom_section_info {
    pub n_rows: u64,
    pub n_calls: u64,
    pub log_n: i32,
    pub defect: i32,
    pub defect_index: u64,
}

/// The five lists of one executed program (mh_miden_chiplets_build): host pointers and counts.
#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct mh_chiplets_lists {
    pub hash_ops: *const mh_hash_op,
    pub n_hash_ops: usize,
    pub hash_felts: *const u64,
    pub n_hash_felts: usize,
    pub bitwise_ops: *const mh_bitwise_op,
    pub n_bitwise_ops: usize,
    pub mem_accesses: *const mh_mem_access,
    pub n_mem_accesses: usize,
    pub ace_evals: *const mh_ace_eval,
    pub n_ace_evals: usize,
    pub ace_felts: *const u64,
    pub n_ace_felts: usize,
    pub kernel_procs: *const u64,
    pub n_kernel_procs: usize,
    pub kernel_calls: *const u64,
    pub n_kernel_calls: usize,
}

/// mh_miden_chiplets_build: the section starts, the trace length, the first defective section (-1 none, 0 hasher .. 4 kernel ROM,
/// 5 the frame) and the five builders' infos.
#[repr(C)]
#[derive(Clone, Copy, Debug, Default, PartialEq, Eq)]
pub struct mh_chiplets_info {
    pub start: [u64; 5],
    pub padding_start: u64,
    pub trace_len: u64,
    pub log_n: i32,
    pub defect_section: i32,
    pub defect: i32,
    pub reserved: i32,
    pub defect_index: u64,
    pub hasher: mh_hasher_section_info,
    pub bitwise: mh_bitwise_section_info,
    pub memory: mh_mem_section_info,
    pub ace: mh_ace_section_info,
    pub kernel_rom: mh_kernel_rom_section_info,
}

/// One message of mh_keccak_traces_build: bytes[offset .. offset + len), chunk_head = the base of its chunk-tape segment in chunks (24 bytes).
#[repr(C)]
#[derive(Clone, Copy, Debug, Default, PartialEq, Eq)]
pub struct mh_keccak_msg {
    pub offset: u64,
    pub len: u64,
    pub chunk_head: u64,
}

/// mh_keccak_traces_build: the permutations, the sponge's active rows, the least heights of both traces, and the defect that refused
/// the call (0 none, 1 offset + len past n_bytes, 2 chunk pointer beyond 32 bits, 3 more than 2^24 rows, 4 a null pointer, 5 / 6
/// log_round / log_sponge too small; see midenhip.h).
#[repr(C)]
#[derive(Clone, Copy, Debug, Default, PartialEq, Eq)]
pub struct mh_keccak_traces_info {
    pub n_perms: u64,
    pub sponge_rows: u64,
    pub round_rows_needed: u64,
    pub sponge_rows_needed: u64,
    pub defect_kind: i32,
    pub defect_index: u64,
}

/// One absorption of mh_poseidon2_chiplet_trace_build: the capacity, the blocks it absorbs and the two multiplicities (56 bytes).
#[repr(C)]
#[derive(Clone, Copy, Debug, Default, PartialEq, Eq)]
pub struct mh_p2c_absorption {
    pub cap: [u64; 4],
    pub n_blocks: u64,
    pub in_mult: u64,
    pub out_mult: u64,
}

/// mh_poseidon2_chiplet_plan / mh_poseidon2_chiplet_trace_build: the ledger's sizes, the least height, the height taken and the defect
/// that refused the call (0 none, 1 a null pointer, 2 n_blocks = 0, 3 the n_blocks do not add up to n_cycles, 4 a bad reference,
/// 5 more than 2^20 cycles, 6 log_n too small; see midenhip.h).
#[repr(C)]
#[derive(Clone, Copy, Debug, Default, PartialEq, Eq)]
pub struct mh_p2c_info {
    pub n_absorptions: u64,
    pub n_cycles: u64,
    pub n_levels: u64,
    pub rows_needed: u64,
    pub log_n: i32,
    pub defect_kind: i32,
    pub defect_index: u64,
}

/// One stored value of mh_uint_traces_build: pointer, bound pointer, eight 32-bit limbs (least first) and the reads of the row from
/// outside the two chiplets (48 bytes).
#[repr(C)]
#[derive(Clone, Copy, Debug, Default, PartialEq, Eq)]
pub struct mh_uint_row {
    pub ptr: u32,
    pub bound_ptr: u32,
    pub value: [u32; 8],
    pub val_reads: u32,
    pub limb_reads: u32,
}

/// kappa_a a b +- kappa_c c = r (mod bound + 1) over store pointers (40 bytes).
#[repr(C)]
#[derive(Clone, Copy, Debug, Default, PartialEq, Eq)]
pub struct mh_uint_mul_op {
    pub a: u32,
    pub b: u32,
    pub c: u32,
    pub r: u32,
    pub bound: u32,
    pub kappa_a: u32,
    pub kappa_c: u32,
    pub is_sub: u32,
    pub mult: u64,
}

/// a + b = c (mod bound + 1) over store pointers; pointer 0 in b or c: absent (32 bytes).
#[repr(C)]
#[derive(Clone, Copy, Debug, Default, PartialEq, Eq)]
pub struct mh_uint_add_op {
    pub a: u32,
    pub b: u32,
    pub c: u32,
    pub bound: u32,
    pub nz: u32,
    pub reserved: u32,
    pub mult: u64,
}

/// mh_uint_traces_plan / mh_uint_traces_build: the lists' sizes, the least heights and the ones taken, and the defect that refused the
/// call: section 0 store, 1 multiply, 2 add; kind 0 none, 1..7 the planner's, 8..14 the device's witness pass (see midenhip.h).
#[repr(C)]
#[derive(Clone, Copy, Debug, Default, PartialEq, Eq)]
pub struct mh_uint_traces_info {
    pub n_store: u64,
    pub n_mul: u64,
    pub n_add: u64,
    pub usm_rows_needed: u64,
    pub usm_rows: u64,
    pub add_rows_needed: u64,
    pub add_rows: u64,
    pub defect_section: i32,
    pub defect_kind: i32,
    pub defect_index: u64,
    pub defect_operand: i32,
    pub reserved: i32,
}

/// One row of the group table of mh_ec_traces_build (group pointer = row + 1): the uint pointers of a, b, the base-field bound and the
/// scalar bound, and the reads of the row from outside the four EC chiplets (24 bytes).
#[repr(C)]
#[derive(Clone, Copy, Debug, Default, PartialEq, Eq)]
pub struct mh_ec_group {
    pub a_ptr: u32,
    pub b_ptr: u32,
    pub bound_ptr: u32,
    pub sbound_ptr: u32,
    pub ext_reads: u64,
}

/// One row of the point store (point pointer = row + 1): kind 0 member (trio u, w), 1 point at infinity, 2 closure-certified (32 bytes).
#[repr(C)]
#[derive(Clone, Copy, Debug, Default, PartialEq, Eq)]
pub struct mh_ec_point {
    pub group: u32,
    pub x_ptr: u32,
    pub y_ptr: u32,
    pub u_ptr: u32,
    pub w_ptr: u32,
    pub kind: u32,
    pub ext_reads: u64,
}

/// p + q = r over point pointers: kind 0 pai_p, 1 pai_q, 2 pai_both, 3 cancel, 4 double, 5 generic; t = slope_aux, lambda, t, y3, e, x3
/// (56 bytes).
#[repr(C)]
#[derive(Clone, Copy, Debug, Default, PartialEq, Eq)]
pub struct mh_ec_add_op {
    pub group: u32,
    pub p: u32,
    pub q: u32,
    pub r: u32,
    pub kind: u32,
    pub mints: u32,
    pub t: [u32; 6],
    pub mult: u64,
}

/// One MSM expression (pointer = index + 1): kind 0 intro, 1 combine, 2 neg (48 bytes).
#[repr(C)]
#[derive(Clone, Copy, Debug, Default, PartialEq, Eq)]
pub struct mh_msm_expr {
    pub kind: u32,
    pub group: u32,
    pub val: u32,
    pub a_expr: u32,
    pub b_expr: u32,
    pub n_rows: u32,
    pub neg_minted: u32,
    pub reserved: u32,
    pub ext_mult: u64,
    pub claim_mult: u64,
}

/// One term row of an MSM expression: the base's point pointer and the scalar's uint pointer (8 bytes).
#[repr(C)]
#[derive(Clone, Copy, Debug, Default, PartialEq, Eq)]
pub struct mh_msm_term {
    pub base: u32,
    pub scalar: u32,
}

/// mh_ec_traces_plan / mh_ec_traces_build: the lists' sizes, the least heights and the ones taken, and the defect that refused the call:
/// section 0 groups, 1 points, 2 add, 3 msm; kind 0 none, 1..7 the planner's, 8..15 the device's checking pass (see midenhip.h).
#[repr(C)]
#[derive(Clone, Copy, Debug, Default, PartialEq, Eq)]
pub struct mh_ec_traces_info {
    pub n_groups: u64,
    pub n_points: u64,
    pub n_add: u64,
    pub n_exprs: u64,
    pub n_terms: u64,
    pub groups_rows_needed: u64,
    pub groups_rows: u64,
    pub points_rows_needed: u64,
    pub points_rows: u64,
    pub add_rows_needed: u64,
    pub add_rows: u64,
    pub msm_rows_needed: u64,
    pub msm_rows: u64,
    pub defect_section: i32,
    pub defect_kind: i32,
    pub defect_index: u64,
    pub defect_operand: i32,
    pub reserved: i32,
}

/// One distinct hashed input of mh_chunk_node_trace_build: where its bytes lie, its chunk chain and sponge rows, the first cycle of the
/// chain's absorption, the one-block absorptions of its digest and of the node, and the node's readers (64 bytes).
#[repr(C)]
#[derive(Clone, Copy, Debug, Default, PartialEq, Eq)]
pub struct mh_kn_record {
    pub offset: u64,
    pub len: u64,
    pub chunk_head: u64,
    pub sponge_head: u64,
    pub perm_chunks: u64,
    pub perm_digest_chunks: u64,
    pub perm_keccak: u64,
    pub out_mult: u64,
}

/// mh_chunk_node_plan / mh_chunk_node_trace_build: sizes, the least height and the one taken, and the defect that refused the call: kind
/// 0 none, 1..7 the planner's, 8, 9 the device's checking pass (see midenhip.h).
#[repr(C)]
#[derive(Clone, Copy, Debug, Default, PartialEq, Eq)]
pub struct mh_chunk_node_info {
    pub n_records: u64,
    pub n_chunks: u64,
    pub p2_cycles: u64,
    pub rows_needed: u64,
    pub rows: u64,
    pub defect_kind: i32,
    pub defect_operand: i32,
    pub defect_index: u64,
}

/// One node of the transcript for mh_transcript_eval_trace_build: kind 0 ZERO, 1 AND, 2 UINT_LEAF, 3 UINT_PIN, 4 UINT_OP, 5 EC_CREATE,
/// 6 EC_PAI, 7 EC_OP, 8 EC_MSM; lhs / rhs a node index below the own, -1 - cycle for an external True binding, a literal index, or an
/// MSM's term_start / n_terms (64 bytes).
#[repr(C)]
#[derive(Clone, Copy, Debug, Default, PartialEq, Eq)]
pub struct mh_te_node {
    pub kind: u32,
    pub op: u32,
    pub lhs: i64,
    pub rhs: i64,
    pub perm: u64,
    pub ptr: u64,
    pub bound_ptr: u64,
    pub group: u64,
    pub expr: u64,
}

/// One term row of an MSM claim: the node indices of its base and its scalar (8 bytes).
#[repr(C)]
#[derive(Clone, Copy, Debug, Default, PartialEq, Eq)]
pub struct mh_te_term {
    pub base_node: u32,
    pub scalar_node: u32,
}

/// mh_transcript_eval_plan / mh_transcript_eval_trace_build: sizes, the active rows, the ZERO nodes other than the root, the heights and
/// the defect that refused the call: kind 0 none, 1..7 the planner's, 8..15 the device's checking pass (see midenhip.h).
#[repr(C)]
#[derive(Clone, Copy, Debug, Default, PartialEq, Eq)]
pub struct mh_transcript_eval_info {
    pub n_nodes: u64,
    pub n_terms: u64,
    pub n_lit: u64,
    pub p2_cycles: u64,
    pub active_rows: u64,
    pub n_zero: u64,
    pub rows_needed: u64,
    pub rows: u64,
    pub defect_kind: i32,
    pub defect_operand: i32,
    pub defect_index: u64,
}

/// An encoded denominator whose net multiplicity is not zero (mh_check_balance*; the reference's `Unmatched`).
#[repr(C)]
#[derive(Clone, Copy, Debug, Default, PartialEq, Eq)]
pub struct mh_balance_entry {
    pub denom: [u64; 2],
    pub net: [u64; 2],
    pub pushes: u64,
    pub first_push: u64,
}

/// A live push that landed on a reported denominator (the reference's `PushRecord` without msg_repr); instance -1: a boundary push.
#[repr(C)]
#[derive(Clone, Copy, Debug, Default, PartialEq, Eq)]
pub struct mh_balance_push {
    pub instance: i32,
    pub column: u32,
    pub fraction: u32,
    pub row: u64,
    pub multiplicity: [u64; 2],
}

/// PcsParams (crates/lifted-stark/src/pcs/params.rs:52-96).
#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct mh_pcs_params {
    pub log_blowup: c_int,
    pub log_folding_arity: c_int,
    pub log_final_degree: c_int,
    pub folding_pow_bits: c_int,
    pub deep_pow_bits: c_int,
    pub num_queries: c_int,
    pub query_pow_bits: c_int,
}

/// LiftedAir::build_aux_trace as a callback (prover/mod.rs:355-381); non-zero aborts the proof.
#[repr(C)]
pub struct mh_local_fabric {
    _private: [u8; 0],
}
pub type mh_aux_builder = Option<
    unsafe extern "C" fn(user: *mut c_void, instance_idx: c_int, randomness: *const u64, aux_out: *mut u64, aux_values_out: *mut u64) -> c_int,
>;
/// Statement::eval_external as a callback (see midenhip.h): writes one EF value per assertion, returns their number or < 0.
pub type mh_external_assertions = Option<
    unsafe extern "C" fn(user: *mut c_void, randomness: *const u64, n_randomness: usize, aux_values: *const *const u64, n_aux_values: *const usize, log_trace_heights: *const u8, n_airs: c_int, assertions_out: *mut u64, cap: usize) -> c_int,
>;

/// One LMCS batch opening as mh_tree_open wrote it (see midenhip.h).
#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct mh_lmcs_opening {
    pub root: [u64; 4],
    pub log_height: c_int,
    pub n_mats: c_int,
    pub widths: *const usize,
    pub alignment: usize,
    pub indices: *const u64,
    pub n_indices: usize,
    pub fields: *const u64,
    pub n_fields: usize,
    pub commitments: *const u64,
    pub n_commit_felts: usize,
}
/// The caller's buffers for one opening of mh_lmcs_witness_batch, sized by mh_lmcs_witness_size; nodes may be null.
#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct mh_lmcs_witness_out {
    pub leaf_digests: *mut u64,
    pub paths: *mut u64,
    pub nodes: *mut u64,
}
/// mh_verify_batch_witness's result: per accepted item one witness per LMCS opening of the proof.
#[repr(C)]
pub struct mh_witness_set {
    _private: [u8; 0],
}
/// One tree of an mh_witness_set; every pointer points into memory the set owns.
#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct mh_witness_tree {
    pub kind: c_int,
    pub which: c_int,
    pub depth: c_int,
    pub n_leaves: usize,
    pub n_nodes: usize,
    pub row_len: usize,
    pub root: [u64; 4],
    pub indices: *const u64,
    pub rows: *const u64,
    pub leaf_digests: *const u64,
    pub paths: *const u64,
    pub nodes: *const u64,
}
/// What differs per proof of an mh_verify_batch call.
#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct mh_verify_item {
    pub log_trace_heights: *const u8,
    pub public_values: *const u64,
    pub n_public_values: usize,
    pub pre_observe: *const u64,
    pub n_pre_observe: usize,
    pub fields: *const u64,
    pub n_fields: usize,
    pub commitments: *const u64,
    pub n_commitments: usize,
    pub preprocessed_root: *const u64,
    pub external_user: *mut c_void,
}
#[repr(C)]
#[derive(Clone, Copy)]
pub struct mh_verify_result {
    pub code: c_int,
    pub digest: [u64; 4],
    pub reason: [c_char; 216],
}
#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct mh_miden_verify_item {
    pub public_values: *const u64,
    pub aux_inputs: *const u64,
    pub n_aux_inputs: usize,
    pub proof_bytes: *const u8,
    pub n_bytes: usize,
}

/// Collectives of a sharded proof, on DEVICE buffers (RCCL): 0 = success.
#[repr(C)]
pub struct mh_comm {
    pub rank: c_int,
    pub world: c_int,
    pub user: *mut c_void,
    pub all_to_all: Option<unsafe extern "C" fn(user: *mut c_void, send_dev: *const c_void, recv_dev: *mut c_void, bytes_per_peer: usize) -> c_int>,
    pub all_gather: Option<unsafe extern "C" fn(user: *mut c_void, send_dev: *const c_void, recv_dev: *mut c_void, bytes_per_rank: usize) -> c_int>,
    pub all_reduce_sum_u64: Option<unsafe extern "C" fn(user: *mut c_void, buf_dev: *mut u64, n: usize) -> c_int>,
    /// 0: host-synchronous callbacks; 1: enqueue on the ctx's stream (the library's own RCCL communicator)
    pub stream_ordered: c_int,
}

#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct mh_session_shape_t {
    pub log_lde_height: c_int,
    pub num_randomness: usize,
    pub num_aux_values: usize,
    pub ood_width: usize,
    pub num_fri_rounds: c_int,
    pub final_poly_len: usize,
}

/// mh_pcs_*: the largest number of points one standalone opening takes
pub const MH_PCS_MAX_POINTS: c_int = 4;
#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct mh_pcs_shape_t {
    pub log_lde_height: c_int,
    pub n_points: c_int,
    pub ood_width: usize,
    pub num_fri_rounds: c_int,
    pub final_poly_len: usize,
}

/// mh_ctx_set_lmcs / mh_verify_lmcs: the StarkConfig (air/src/config.rs:212-353) by its hash function
pub const MH_LMCS_POSEIDON2: c_int = 0;
pub const MH_LMCS_BLAKE3: c_int = 1;
pub const MH_LMCS_KECCAK: c_int = 2;
pub const MH_LMCS_RPO: c_int = 3;
pub const MH_LMCS_RPX: c_int = 4;
/// mh_ctx_set_salt: the largest salt width (felts per leaf) of the hiding LMCS
pub const MH_MAX_SALT_ELEMS: c_int = 8;

#[link(name = "midenhip")]
unsafe extern "C" {
    // ---- context ----
    pub fn mh_ctx_create(device_id: c_int, out: *mut *mut mh_ctx) -> c_int;
    pub fn mh_ctx_destroy(ctx: *mut mh_ctx);
    pub fn mh_ctx_trim(ctx: *mut mh_ctx) -> c_int;
    /// out = [pool bytes, table bytes, device free, device total]
    pub fn mh_ctx_mem_stats(ctx: *mut mh_ctx, out: *mut u64) -> c_int;
    pub fn mh_last_error(ctx: *const mh_ctx) -> *const c_char;
    pub fn mh_device_count() -> c_int;
    /// MH_LMCS_POSEIDON2 = 0, MH_LMCS_BLAKE3 = 1 (the hasher of mh_commit_traces / mh_tree_open on this context)
    pub fn mh_ctx_set_lmcs(ctx: *mut mh_ctx, lmcs: c_int) -> c_int;
    pub fn mh_ctx_get_lmcs(ctx: *const mh_ctx) -> c_int;
    /// hiding LMCS (lmcs/hiding_config.rs): salt_elems = 0 (off) ..= 8; seed = [u64; 4], secret and fresh per proof, or null (OS entropy)
    pub fn mh_ctx_set_salt(ctx: *mut mh_ctx, salt_elems: c_int, seed: *const u64) -> c_int;
    pub fn mh_ctx_get_salt(ctx: *const mh_ctx) -> c_int;
    pub fn mh_blake3(data: *const u8, n: usize, out32: *mut u8);
    pub fn mh_prof_enable(ctx: *mut mh_ctx, on: c_int) -> c_int;
    pub fn mh_prof_filter(ctx: *mut mh_ctx, name: *const c_char) -> c_int;
    pub fn mh_prof_reset(ctx: *mut mh_ctx) -> c_int;
    pub fn mh_prof_get(ctx: *mut mh_ctx, name: *const c_char, ms: *mut c_double, bytes: *mut c_double, count: *mut c_long) -> c_int;
    pub fn mh_prof_dump(ctx: *mut mh_ctx, buf: *mut c_char, cap: usize) -> c_int;
    // ---- unit-parity entry points ----
    pub fn mh_poseidon2_permute(ctx: *mut mh_ctx, states: *mut u64, n: usize) -> c_int;
    pub fn mh_poseidon2_register_rate(ctx: *mut mh_ctx, perms_per_second: *mut c_double) -> c_int;
    pub fn mh_coset_lde_batch(ctx: *mut mh_ctx, rowmajor: *const u64, log_n: c_int, width: usize, added_bits: c_int, shift: u64, out: *mut u64) -> c_int;
    // ---- traces ----
    pub fn mh_trace_upload(ctx: *mut mh_ctx, rowmajor: *const u64, log_n: c_int, width: usize, out: *mut *mut mh_trace) -> c_int;
    pub fn mh_trace_upload_async(ctx: *mut mh_ctx, rowmajor: *const u64, log_n: c_int, width: usize, out: *mut *mut mh_trace) -> c_int;
    pub fn mh_trace_upload_cols_async(ctx: *mut mh_ctx, colmajor: *const u64, log_n: c_int, width: usize, out: *mut *mut mh_trace) -> c_int;
    pub fn mh_trace_wait(ctx: *mut mh_ctx, t: *mut mh_trace) -> c_int;
    pub fn mh_trace_from_device(ctx: *mut mh_ctx, device_rowmajor: *const u64, log_n: c_int, width: usize, out: *mut *mut mh_trace) -> c_int;
    pub fn mh_trace_download(ctx: *mut mh_ctx, t: *const mh_trace, rowmajor_out: *mut u64) -> c_int;
    pub fn mh_trace_free(t: *mut mh_trace);
    pub fn mh_host_alloc(bytes: usize) -> *mut c_void;
    pub fn mh_host_free(p: *mut c_void);
    // ---- commitments ----
    pub fn mh_commit_traces(ctx: *mut mh_ctx, n_traces: c_int, traces: *const *mut mh_trace, log_blowup: c_int, out: *mut *mut mh_tree, root: *mut u64) -> c_int;
    /// host only (no context, no GPU): mh_commit_traces' root from row-major host matrices -- the verifier's way to a preprocessed_root
    pub fn mh_commit_host(lmcs: c_int, n_mats: c_int, rowmajor: *const *const u64, log_heights: *const u8, widths: *const usize, log_blowup: c_int, root: *mut u64, err: *mut c_char, err_cap: usize) -> c_int;
    pub fn mh_tree_free(t: *mut mh_tree);
    pub fn mh_tree_root(t: *const mh_tree, root: *mut u64) -> c_int;
    pub fn mh_tree_log_height(t: *const mh_tree) -> c_int;
    pub fn mh_tree_open(ctx: *mut mh_ctx, t: *const mh_tree, indices: *const u64, n_idx: usize, alignment: usize, fields: *mut u64, n_fields: *mut usize, commits: *mut u64, n_commit_felts: *mut usize) -> c_int;
    pub fn mh_tree_download_lde(ctx: *mut mh_ctx, t: *const mh_tree, mat: c_int, out_rowmajor_bitrev: *mut u64) -> c_int;
    pub fn mh_tree_download_layers(ctx: *mut mh_ctx, t: *const mh_tree, out: *mut u64) -> c_int;
    pub fn mh_tree_salt_elems(t: *const mh_tree) -> c_int;
    pub fn mh_tree_salt_index(t: *const mh_tree) -> u64;
    /// out = [2^log_height][salt_elems], physical (bit-reversed) row order
    pub fn mh_tree_download_salt(ctx: *mut mh_ctx, t: *const mh_tree, out: *mut u64) -> c_int;
    pub fn mh_shard_commit_leaves(ctx: *mut mh_ctx, n_traces: c_int, traces: *const *mut mh_trace, log_blowup: c_int, rank: c_int, world: c_int, out: *mut *mut mh_shard) -> c_int;
    pub fn mh_shard_free(s: *mut mh_shard);
    pub fn mh_shard_leaf_digests(s: *mut mh_shard, n_digests: *mut usize) -> *mut u64;
    pub fn mh_shard_build_subtree(ctx: *mut mh_ctx, s: *mut mh_shard, digests_device: *const u64, subroot: *mut u64) -> c_int;
    pub fn mh_merkle_cap_root(subroots: *const u64, world: c_int, root: *mut u64) -> c_int;
    pub fn mh_merkle_cap_root_lmcs(lmcs: c_int, subroots: *const u64, world: c_int, root: *mut u64) -> c_int;
    // ---- AIRs, lookups ----
    pub fn mh_air_load(ctx: *mut mh_ctx, blob: *const u64, n_words: usize, out: *mut *mut mh_air) -> c_int;
    pub fn mh_air_free(air: *mut mh_air);
    pub fn mh_air_log_quotient_degree(air: *const mh_air) -> c_int;
    pub fn mh_air_compiled_chunks(air: *const mh_air) -> c_int;
    pub fn mh_air_compiled_max_vgprs(air: *const mh_air) -> c_int;
    pub fn mh_jit_precompile(blob: *const u64, n_words: usize, n_chunks: *mut c_int) -> c_int;
    pub fn mh_air_attach_preprocessed(air: *mut mh_air, tree: *const mh_tree, matrix_index: c_int, raw: *const mh_trace) -> c_int;
    pub fn mh_air_attach_lookup(air: *mut mh_air, l: *const mh_lookup) -> c_int;
    pub fn mh_lookup_load(ctx: *mut mh_ctx, blob: *const u64, n_words: usize, out: *mut *mut mh_lookup) -> c_int;
    pub fn mh_lookup_free(l: *mut mh_lookup);
    pub fn mh_lookup_build_aux(ctx: *mut mh_ctx, l: *const mh_lookup, main_trace: *const mh_trace, preprocessed: *const mh_trace, randomness: *const u64, n_randomness: usize, aux_out: *mut *mut mh_trace, acc_final: *mut u64) -> c_int;
    // ---- proofs ----
    pub fn mh_prove(ctx: *mut mh_ctx, params: *const mh_pcs_params, n_airs: c_int, airs: *const *mut mh_air, traces: *const *mut mh_trace, public_values: *const u64, n_public_values: usize, challenger_state: *const u64, pre_observe: *const u64, n_pre_observe: usize, aux_builder: mh_aux_builder, user: *mut c_void, out: *mut *mut mh_proof) -> c_int;
    pub fn mh_commit_traces_sharded(ctx: *mut mh_ctx, comm: *const mh_comm, n_traces: c_int, traces: *const *mut mh_trace, log_blowup: c_int, out: *mut *mut mh_tree, root: *mut u64) -> c_int;
    pub fn mh_prove_host(ctx: *mut mh_ctx, params: *const mh_pcs_params, n_airs: c_int, airs: *const *mut mh_air, traces_rowmajor: *const *const u64,
                         log_heights: *const c_int, public_values: *const u64, n_public_values: usize, challenger_state: *const u64,
                         pre_observe: *const u64, n_pre_observe: usize, aux_builder: mh_aux_builder, user: *mut c_void, out: *mut *mut mh_proof) -> c_int;
    pub fn mh_prove_sharded(ctx: *mut mh_ctx, comm: *const mh_comm, params: *const mh_pcs_params, n_airs: c_int, airs: *const *mut mh_air, traces: *const *mut mh_trace, public_values: *const u64, n_public_values: usize, challenger_state: *const u64, pre_observe: *const u64, n_pre_observe: usize, aux_builder: mh_aux_builder, user: *mut c_void, out: *mut *mut mh_proof) -> c_int;
    pub fn mh_session_begin(ctx: *mut mh_ctx, comm: *const mh_comm, params: *const mh_pcs_params, n_airs: c_int, airs: *const *mut mh_air, traces: *const *mut mh_trace, public_values: *const u64, n_public_values: usize, out: *mut *mut mh_session) -> c_int;
    pub fn mh_session_free(s: *mut mh_session);
    pub fn mh_session_shape(s: *const mh_session, out: *mut mh_session_shape_t) -> c_int;
    pub fn mh_session_commit_main(s: *mut mh_session, root: *mut u64) -> c_int;
    pub fn mh_session_commit_aux(s: *mut mh_session, randomness: *const u64, aux_builder: mh_aux_builder, user: *mut c_void, root: *mut u64, aux_values_out: *mut u64) -> c_int;
    pub fn mh_session_commit_quotient(s: *mut mh_session, alpha: *const u64, beta: *const u64, root: *mut u64) -> c_int;
    pub fn mh_session_ood_point_ok(s: *const mh_session, z: *const u64) -> c_int;
    pub fn mh_session_ood(s: *mut mh_session, z: *const u64, evals_out: *mut u64) -> c_int;
    pub fn mh_session_deep(s: *mut mh_session, alpha: *const u64, beta: *const u64) -> c_int;
    pub fn mh_session_fri_commit(s: *mut mh_session, root: *mut u64) -> c_int;
    pub fn mh_session_fri_fold(s: *mut mh_session, beta: *const u64) -> c_int;
    pub fn mh_session_fri_final(s: *mut mh_session, coeffs_out: *mut u64) -> c_int;
    pub fn mh_session_open(s: *mut mh_session, indices: *const u64, n_indices: usize, out: *mut *mut mh_proof) -> c_int;
    /// out: room for `cap` borrowed trees, group order [preprocessed?, main, aux, quotient]; valid once the quotient is committed
    pub fn mh_session_trees(s: *const mh_session, out: *mut *const mh_tree, cap: c_int, n_trees: *mut c_int) -> c_int;
    // ---- the PCS on its own: pcs::open_with_channel / pcs::verify_aligned over any trees and 1..=4 points ----
    /// host only: 1 = z = [c0, c1] is nonzero, outside H and outside gK
    pub fn mh_pcs_point_ok(log_max_trace_height: c_int, log_blowup: c_int, z: *const u64) -> c_int;
    /// borrows the trees; points = [n_points][2]
    pub fn mh_pcs_begin(ctx: *mut mh_ctx, params: *const mh_pcs_params, n_trees: c_int, trees: *const *const mh_tree, n_points: c_int, points: *const u64, out: *mut *mut mh_pcs) -> c_int;
    pub fn mh_pcs_free(p: *mut mh_pcs);
    pub fn mh_pcs_shape(p: *const mh_pcs, out: *mut mh_pcs_shape_t) -> c_int;
    /// evals_out = [n_points][ood_width][2], transcript order
    pub fn mh_pcs_evals(p: *mut mh_pcs, evals_out: *mut u64) -> c_int;
    pub fn mh_pcs_deep(p: *mut mh_pcs, alpha: *const u64, beta: *const u64) -> c_int;
    /// parity/debug: [2^log_lde_height][2], domain order
    pub fn mh_pcs_download_deep(p: *mut mh_pcs, out: *mut u64) -> c_int;
    pub fn mh_pcs_fri_commit(p: *mut mh_pcs, root: *mut u64) -> c_int;
    pub fn mh_pcs_fri_fold(p: *mut mh_pcs, beta: *const u64) -> c_int;
    pub fn mh_pcs_fri_final(p: *mut mh_pcs, coeffs_out: *mut u64) -> c_int;
    /// hints only, like mh_session_open
    pub fn mh_pcs_query(p: *mut mh_pcs, indices: *const u64, n_indices: usize, out: *mut *mut mh_proof) -> c_int;
    /// one shot, library-owned transcript; the roots are the caller's to bind (pre_observe)
    pub fn mh_pcs_open(ctx: *mut mh_ctx, params: *const mh_pcs_params, n_trees: c_int, trees: *const *const mh_tree, n_points: c_int, points: *const u64, challenger_state: *const u64, pre_observe: *const u64, n_pre_observe: usize, out: *mut *mut mh_proof) -> c_int;
    /// host only; roots = [n_trees][4], widths = unpadded, all trees flat; evals_out may be null
    pub fn mh_pcs_verify(lmcs: c_int, salt_elems: c_int, params: *const mh_pcs_params, n_trees: c_int, roots: *const u64, log_tree_heights: *const u8, n_mats: *const c_int, widths: *const usize, n_points: c_int, points: *const u64, challenger_state: *const u64, pre_observe: *const u64, n_pre_observe: usize, fields: *const u64, n_fields: usize, commitments: *const u64, n_commitments: usize, evals_out: *mut u64, digest: *mut u64, err: *mut c_char, err_cap: usize) -> c_int;
    pub fn mh_grind(ctx: *mut mh_ctx, state: *const u64, pending: *const u64, n_pending: usize, bits: c_int, witness: *mut u64) -> c_int;
    pub fn mh_grind_bytes(ctx: *mut mh_ctx, input: *const u8, n_input: usize, bits: c_int, witness: *mut u64) -> c_int;
    pub fn mh_verify(params: *const mh_pcs_params, n_airs: c_int, air_blobs: *const *const u64, air_blob_words: *const usize, log_trace_heights: *const u8, public_values: *const u64, n_public_values: usize, challenger_state: *const u64, pre_observe: *const u64, n_pre_observe: usize, fields: *const u64, n_fields: usize, commitments: *const u64, n_commitments: usize, preprocessed_root: *const u64, digest: *mut u64, err: *mut c_char, err_cap: usize) -> c_int;
    pub fn mh_verify_ex(params: *const mh_pcs_params, n_airs: c_int, air_blobs: *const *const u64, air_blob_words: *const usize, log_trace_heights: *const u8, public_values: *const u64, n_public_values: usize, challenger_state: *const u64, pre_observe: *const u64, n_pre_observe: usize, fields: *const u64, n_fields: usize, commitments: *const u64, n_commitments: usize, preprocessed_root: *const u64, external: mh_external_assertions, external_user: *mut c_void, digest: *mut u64, err: *mut c_char, err_cap: usize) -> c_int;
    /// mh_verify_ex for MH_LMCS_RPO (3) / MH_LMCS_RPX (4) / MH_LMCS_POSEIDON2 (0)
    pub fn mh_verify_lmcs(lmcs: c_int, params: *const mh_pcs_params, n_airs: c_int, air_blobs: *const *const u64, air_blob_words: *const usize, log_trace_heights: *const u8, public_values: *const u64, n_public_values: usize, challenger_state: *const u64, pre_observe: *const u64, n_pre_observe: usize, fields: *const u64, n_fields: usize, commitments: *const u64, n_commitments: usize, preprocessed_root: *const u64, external: mh_external_assertions, external_user: *mut c_void, digest: *mut u64, err: *mut c_char, err_cap: usize) -> c_int;
    /// mh_verify_lmcs for a proof made under a hiding LMCS (mh_ctx_set_salt): salt_elems salt felts follow every opened leaf
    pub fn mh_verify_hiding(lmcs: c_int, salt_elems: c_int, params: *const mh_pcs_params, n_airs: c_int, air_blobs: *const *const u64, air_blob_words: *const usize, log_trace_heights: *const u8, public_values: *const u64, n_public_values: usize, challenger_state: *const u64, pre_observe: *const u64, n_pre_observe: usize, fields: *const u64, n_fields: usize, commitments: *const u64, n_commitments: usize, preprocessed_root: *const u64, external: mh_external_assertions, external_user: *mut c_void, digest: *mut u64, err: *mut c_char, err_cap: usize) -> c_int;
    pub fn mh_external_logup_balance(user: *mut c_void, randomness: *const u64, n_randomness: usize, aux_values: *const *const u64, n_aux_values: *const usize, log_trace_heights: *const u8, n_airs: c_int, assertions_out: *mut u64, cap: usize) -> c_int;
    pub fn mh_external_precompile_session(user: *mut c_void, randomness: *const u64, n_randomness: usize, aux_values: *const *const u64, n_aux_values: *const usize, log_trace_heights: *const u8, n_airs: c_int, assertions_out: *mut u64, cap: usize) -> c_int;
    pub fn mh_external_precompile_session_ec_only(user: *mut c_void, randomness: *const u64, n_randomness: usize, aux_values: *const *const u64, n_aux_values: *const usize, log_trace_heights: *const u8, n_airs: c_int, assertions_out: *mut u64, cap: usize) -> c_int;
    // the precompile prover's session: SessionTraces::prove_stark's own shape (csrc/precompile.cpp)
    pub fn mh_precompile_pcs_params(out: *mut mh_pcs_params);
    pub fn mh_precompile_load(ctx: *mut mh_ctx, out: *mut *mut mh_precompile) -> c_int;
    pub fn mh_precompile_free(s: *mut mh_precompile);
    pub fn mh_precompile_air_blob(which: c_int, lookup: c_int, words_out: *mut *const u64, n_words: *mut usize) -> c_int;
    pub fn mh_precompile_preprocessed_root(s: *mut mh_precompile, hash_fn: c_int, root: *mut u64) -> c_int;
    /// host only: the byte-pair table's setup commitment derived from the table (cached per hash function)
    pub fn mh_precompile_setup_root(hash_fn: c_int, root: *mut u64) -> c_int;
    pub fn mh_precompile_pre_observe(p: *const mh_pcs_params, preprocessed_root: *const u64, public_root: *const u64, out: *mut u64) -> c_int;
    pub fn mh_prove_precompile(ctx: *mut mh_ctx, s: *mut mh_precompile, hash_fn: c_int, mains_rowmajor: *const *const u64, log_heights: *const c_int, public_root: *const u64, out: *mut *mut mh_proof) -> c_int;
    pub fn mh_prove_precompile_traces(ctx: *mut mh_ctx, s: *mut mh_precompile, hash_fn: c_int, traces: *const *mut mh_trace, public_root: *const u64, out: *mut *mut mh_proof) -> c_int;
    /// preprocessed_root: null = derive it (mh_precompile_setup_root); non-null = checked against the derived root first
    pub fn mh_verify_precompile(hash_fn: c_int, preprocessed_root: *const u64, public_root: *const u64, proof_bytes: *const u8, n_bytes: usize, digest: *mut u64, err: *mut c_char, err_cap: usize) -> c_int;
    pub fn mh_proof_deserialize(bytes: *const u8, len: usize, out: *mut *mut mh_proof) -> c_int;
    pub fn mh_trace_upload_sharded(ctx: *mut mh_ctx, comm: *const mh_comm, rowmajor: *const u64, log_n: c_int, width: usize, out: *mut *mut mh_trace) -> c_int;
    pub fn mh_rccl_unique_id(id: *mut u8) -> c_int;
    pub fn mh_comm_create_rccl(ctx: *mut mh_ctx, id: *const u8, rank: c_int, world: c_int, out: *mut *mut mh_comm) -> c_int;
    pub fn mh_comm_destroy(comm: *mut mh_comm);
    pub fn mh_local_fabric_create(world: c_int) -> *mut mh_local_fabric;
    pub fn mh_local_fabric_destroy(f: *mut mh_local_fabric);
    pub fn mh_local_fabric_abort(f: *mut mh_local_fabric);
    pub fn mh_comm_create_local(ctx: *mut mh_ctx, f: *mut mh_local_fabric, rank: c_int, out: *mut *mut mh_comm) -> c_int;
    pub fn mh_comm_selftest(ctx: *mut mh_ctx, comm: *const mh_comm) -> c_int;
    // ---- the Miden statement in the library (prove_stark's own shape, prover/src/lib.rs:317-355); a Rust shim that keeps
    // `MidenMultiAir` on its side uses mh_prove / mh_verify_ex instead
    pub fn mh_miden_load(ctx: *mut mh_ctx, out: *mut *mut mh_miden) -> c_int;
    pub fn mh_miden_free(m: *mut mh_miden);
    pub fn mh_prove_miden(ctx: *mut mh_ctx, m: *const mh_miden, hash_fn: c_int, core_rowmajor: *const u64, log_core: c_int, chiplets_rowmajor: *const u64, log_chiplets: c_int, poseidon2_rowmajor: *const u64, log_poseidon2: c_int, public_values: *const u64, aux_inputs: *const u64, n_aux_inputs: usize, out: *mut *mut mh_proof) -> c_int;
    pub fn mh_prove_miden_traces(ctx: *mut mh_ctx, m: *const mh_miden, hash_fn: c_int, traces: *const *mut mh_trace, public_values: *const u64, aux_inputs: *const u64, n_aux_inputs: usize, out: *mut *mut mh_proof) -> c_int;
    pub fn mh_verify_miden(hash_fn: c_int, public_values: *const u64, aux_inputs: *const u64, n_aux_inputs: usize, proof_bytes: *const u8, n_bytes: usize, digest: *mut u64, err: *mut c_char, err_cap: usize) -> c_int;
    /// mh_verify_miden for n proofs through mh_verify_batch; results[i] as mh_verify_batch fills them
    pub fn mh_verify_miden_batch(ctx: *mut mh_ctx, hash_fn: c_int, n: usize, items: *const mh_miden_verify_item, results: *mut mh_verify_result) -> c_int;
    // ---- LMCS openings on their own (the counterpart of mh_tree_open) and the batch verifier ----
    /// host only, no context
    pub fn mh_lmcs_verify(lmcs: c_int, salt_elems: c_int, o: *const mh_lmcs_opening, err: *mut c_char, err_cap: usize) -> c_int;
    /// the same for n openings on the device; ok[i] = 1 iff mh_lmcs_verify accepts items[i]
    pub fn mh_lmcs_verify_batch(ctx: *mut mh_ctx, lmcs: c_int, salt_elems: c_int, n: usize, items: *const mh_lmcs_opening, ok: *mut c_int) -> c_int;
    /// mh_verify_hiding for many proofs of one statement shape: host replay per item, every opening hashed on the device
    pub fn mh_verify_batch(ctx: *mut mh_ctx, lmcs: c_int, salt_elems: c_int, params: *const mh_pcs_params, n_airs: c_int, air_blobs: *const *const u64, air_blob_words: *const usize, challenger_state: *const u64, external: mh_external_assertions, n_items: usize, items: *const mh_verify_item, results: *mut mh_verify_result) -> c_int;
    /// an opening read back as a Merkle witness: shape only (any index order, duplicates allowed)
    pub fn mh_lmcs_witness_size(o: *const mh_lmcs_opening, n_leaves: *mut usize, n_nodes: *mut usize, err: *mut c_char, err_cap: usize) -> c_int;
    /// host only: leaf_digests[k][4], paths[k][depth][4], nodes[n_nodes][4] (or null); MH_OK exactly when mh_lmcs_verify accepts
    pub fn mh_lmcs_witness(lmcs: c_int, salt_elems: c_int, o: *const mh_lmcs_opening, leaf_digests: *mut u64, paths: *mut u64, nodes: *mut u64, err: *mut c_char, err_cap: usize) -> c_int;
    /// the same for n openings on the device; for ok[i] = 0 the item's buffers are untouched
    pub fn mh_lmcs_witness_batch(ctx: *mut mh_ctx, lmcs: c_int, salt_elems: c_int, n: usize, items: *const mh_lmcs_opening, outs: *const mh_lmcs_witness_out, ok: *mut c_int) -> c_int;
    /// mh_verify_batch that hands back the witnesses of every accepted item's openings, in proof order
    pub fn mh_verify_batch_witness(ctx: *mut mh_ctx, lmcs: c_int, salt_elems: c_int, params: *const mh_pcs_params, n_airs: c_int, air_blobs: *const *const u64, air_blob_words: *const usize, challenger_state: *const u64, external: mh_external_assertions, n_items: usize, items: *const mh_verify_item, results: *mut mh_verify_result, out: *mut *mut mh_witness_set) -> c_int;
    pub fn mh_witness_set_trees(set: *const mh_witness_set, item: usize) -> usize;
    pub fn mh_witness_set_tree(set: *const mh_witness_set, item: usize, t: usize, view: *mut mh_witness_tree) -> c_int;
    pub fn mh_witness_set_free(set: *mut mh_witness_set);
    pub fn mh_verify_miden_batch_witness(ctx: *mut mh_ctx, hash_fn: c_int, n: usize, items: *const mh_miden_verify_item, results: *mut mh_verify_result, out: *mut *mut mh_witness_set) -> c_int;
    pub fn mh_miden_pcs_params(out: *mut mh_pcs_params);
    pub fn mh_miden_challenger_state(state: *mut u64);
    pub fn mh_miden_hash_kernel_digests(kernel_felts: *const u64, n_felts: usize, out: *mut u64) -> c_int;
    pub fn mh_miden_pre_observe(params: *const mh_pcs_params, public_values: *const u64, aux_inputs: *const u64, n_aux_inputs: usize, out: *mut u64) -> c_int;
    pub fn mh_miden_eval_external(randomness: *const u64, aux_inputs: *const u64, n_aux_inputs: usize, aux_values: *const *const u64, n_aux_values: *const usize, n_airs: c_int, out: *mut u64) -> c_int;
    pub fn mh_miden_air_blob(which: c_int, words_out: *mut *const u64, n_words: *mut usize) -> c_int;
    pub fn mh_proof_free(p: *mut mh_proof);
    pub fn mh_proof_num_fields(p: *const mh_proof) -> usize;
    pub fn mh_proof_num_commitments(p: *const mh_proof) -> usize;
    pub fn mh_proof_fields(p: *const mh_proof) -> *const u64;
    pub fn mh_proof_commitments(p: *const mh_proof) -> *const u64;
    pub fn mh_proof_digest(p: *const mh_proof) -> *const u64;
    pub fn mh_proof_num_traces(p: *const mh_proof) -> usize;
    pub fn mh_proof_log_trace_heights(p: *const mh_proof) -> *const u8;
    pub fn mh_proof_serialize(p: *const mh_proof, out: *mut u8, cap: usize) -> usize;
    // ---- constraint checker (ExecutionTrace::check_constraints, SessionTraces::check): MH_OK or MH_ERR_UNSATISFIED + the entries
    pub fn mh_check_constraints(ctx: *mut mh_ctx, air: *const mh_air, main_trace: *const mh_trace, aux: *const mh_trace, preprocessed: *const mh_trace, public_values: *const u64, n_public: usize, randomness: *const u64, n_randomness: usize, aux_values: *const u64, n_aux_values: usize, flags: c_int, out: *mut mh_check_entry, cap: usize, n_entries: *mut usize, failing_rows: *mut u64) -> c_int;
    pub fn mh_constraint_fold(ctx: *mut mh_ctx, air: *const mh_air, main_trace: *const mh_trace, aux: *const mh_trace, preprocessed: *const mh_trace, public_values: *const u64, n_public: usize, randomness: *const u64, n_randomness: usize, aux_values: *const u64, n_aux_values: usize, alpha: *const u64, out: *mut u64) -> c_int;
    pub fn mh_check_miden(ctx: *mut mh_ctx, m: *const mh_miden, core_rowmajor: *const u64, log_core: c_int, chiplets_rowmajor: *const u64, log_chiplets: c_int, poseidon2_rowmajor: *const u64, log_poseidon2: c_int, public_values: *const u64, aux_inputs: *const u64, n_aux_inputs: usize, flags: c_int, out: *mut mh_check_entry, cap: usize, n_entries: *mut usize) -> c_int;
    pub fn mh_check_miden_traces(ctx: *mut mh_ctx, m: *const mh_miden, traces: *const *mut mh_trace, public_values: *const u64, aux_inputs: *const u64, n_aux_inputs: usize, flags: c_int, out: *mut mh_check_entry, cap: usize, n_entries: *mut usize) -> c_int;
    pub fn mh_check_precompile(ctx: *mut mh_ctx, s: *mut mh_precompile, mains_rowmajor: *const *const u64, log_heights: *const c_int, public_root: *const u64, flags: c_int, out: *mut mh_check_entry, cap: usize, n_entries: *mut usize) -> c_int;
    pub fn mh_check_precompile_traces(ctx: *mut mh_ctx, s: *mut mh_precompile, traces: *const *mut mh_trace, public_root: *const u64, flags: c_int, out: *mut mh_check_entry, cap: usize, n_entries: *mut usize) -> c_int;
    pub fn mh_check_balance(ctx: *mut mh_ctx, n: c_int, lookups: *const *const mh_lookup, traces: *const *const mh_trace, preprocessed: *const *const mh_trace, randomness: *const u64, n_randomness: usize, boundary_denoms: *const u64, boundary_signs: *const i32, n_boundary: usize, flags: c_int, entries: *mut mh_balance_entry, entry_cap: usize, n_entries: *mut usize, pushes: *mut mh_balance_push, push_cap: usize, n_pushes: *mut usize) -> c_int;
    pub fn mh_check_balance_miden(ctx: *mut mh_ctx, m: *const mh_miden, core_rowmajor: *const u64, log_core: c_int, chiplets_rowmajor: *const u64, log_chiplets: c_int, poseidon2_rowmajor: *const u64, log_poseidon2: c_int, public_values: *const u64, aux_inputs: *const u64, n_aux_inputs: usize, flags: c_int, entries: *mut mh_balance_entry, entry_cap: usize, n_entries: *mut usize, pushes: *mut mh_balance_push, push_cap: usize, n_pushes: *mut usize) -> c_int;
    pub fn mh_check_balance_miden_traces(ctx: *mut mh_ctx, m: *const mh_miden, traces: *const *mut mh_trace, public_values: *const u64, aux_inputs: *const u64, n_aux_inputs: usize, flags: c_int, entries: *mut mh_balance_entry, entry_cap: usize, n_entries: *mut usize, pushes: *mut mh_balance_push, push_cap: usize, n_pushes: *mut usize) -> c_int;
    pub fn mh_check_balance_precompile(ctx: *mut mh_ctx, s: *mut mh_precompile, mains_rowmajor: *const *const u64, log_heights: *const c_int, public_root: *const u64, flags: c_int, entries: *mut mh_balance_entry, entry_cap: usize, n_entries: *mut usize, pushes: *mut mh_balance_push, push_cap: usize, n_pushes: *mut usize) -> c_int;
    pub fn mh_check_balance_precompile_traces(ctx: *mut mh_ctx, s: *mut mh_precompile, traces: *const *mut mh_trace, public_root: *const u64, flags: c_int, entries: *mut mh_balance_entry, entry_cap: usize, n_entries: *mut usize, pushes: *mut mh_balance_push, push_cap: usize, n_pushes: *mut usize) -> c_int;
    // multiplicity columns filled on the device, in place (csrc/multiplicity.hip); the report is mh_check_balance's exact stage
    pub fn mh_fill_multiplicities(ctx: *mut mh_ctx, n: c_int, lookups: *const *const mh_lookup, traces: *const *mut mh_trace, preprocessed: *const *const mh_trace, randomness: *const u64, n_randomness: usize, boundary_denoms: *const u64, boundary_signs: *const i32, n_boundary: usize, slots: *const mh_mult_slot, n_slots: usize, n_written: *mut u64, entries: *mut mh_balance_entry, entry_cap: usize, n_entries: *mut usize, pushes: *mut mh_balance_push, push_cap: usize, n_pushes: *mut usize) -> c_int;
    pub fn mh_fill_multiplicities_miden_traces(ctx: *mut mh_ctx, m: *const mh_miden, traces: *const *mut mh_trace, public_values: *const u64, aux_inputs: *const u64, n_aux_inputs: usize, slots: *const mh_mult_slot, n_slots: usize, n_written: *mut u64, entries: *mut mh_balance_entry, entry_cap: usize, n_entries: *mut usize, pushes: *mut mh_balance_push, push_cap: usize, n_pushes: *mut usize) -> c_int;
    pub fn mh_fill_multiplicities_precompile_traces(ctx: *mut mh_ctx, s: *mut mh_precompile, traces: *const *mut mh_trace, public_root: *const u64, slots: *const mh_mult_slot, n_slots: usize, n_written: *mut u64, entries: *mut mh_balance_entry, entry_cap: usize, n_entries: *mut usize, pushes: *mut mh_balance_push, push_cap: usize, n_pushes: *mut usize) -> c_int;
    // the Poseidon2 permutation trace of the Miden statement, built on the device (csrc/p2_trace.hip); info may be null
    pub fn mh_poseidon2_trace_build(ctx: *mut mh_ctx, states: *const u64, multiplicities: *const u64, k: usize, log_n: c_int, out: *mut *mut mh_trace, info: *mut mh_p2_trace_info) -> c_int;
    pub fn mh_miden_poseidon2_trace(ctx: *mut mh_ctx, chiplets: *const mh_trace, log_n: c_int, out: *mut *mut mh_trace, info: *mut mh_p2_trace_info) -> c_int;
    // the range-check table laid on the device from the statement's lookups, in place (csrc/range_table.hip); info may be null
    pub fn mh_fill_range_table(ctx: *mut mh_ctx, n: c_int, lookups: *const *const mh_lookup, traces: *const *mut mh_trace, preprocessed: *const *const mh_trace, randomness: *const u64, n_randomness: usize, boundary_denoms: *const u64, boundary_signs: *const i32, n_boundary: usize, slot: *const mh_range_slot, info: *mut mh_range_table_info, n_written: *mut u64, entries: *mut mh_balance_entry, entry_cap: usize, n_entries: *mut usize, pushes: *mut mh_balance_push, push_cap: usize, n_pushes: *mut usize) -> c_int;
    pub fn mh_fill_range_table_miden_traces(ctx: *mut mh_ctx, m: *const mh_miden, traces: *const *mut mh_trace, public_values: *const u64, aux_inputs: *const u64, n_aux_inputs: usize, info: *mut mh_range_table_info, n_written: *mut u64, entries: *mut mh_balance_entry, entry_cap: usize, n_entries: *mut usize, pushes: *mut mh_balance_push, push_cap: usize, n_pushes: *mut usize) -> c_int;
    // the memory chiplet's trace section built on the device from an access list (csrc/memory_section.hip); row_of and info may be null
    pub fn mh_memory_section_build(ctx: *mut mh_ctx, accesses: *const mh_mem_access, n: usize, log_n: c_int, out: *mut *mut mh_trace, row_of: *mut u32, info: *mut mh_mem_section_info) -> c_int;
    pub fn mh_miden_memory_section(ctx: *mut mh_ctx, chiplets: *mut mh_trace, start_row: u64, accesses: *const mh_mem_access, n: usize, row_of: *mut u32, info: *mut mh_mem_section_info) -> c_int;
    pub fn mh_memory_section_tile() -> u32;
    // the hasher controller's trace section built on the device from an op list (csrc/hasher_section.hip); results and info may be null
    pub fn mh_hasher_section_build(ctx: *mut mh_ctx, ops: *const mh_hash_op, n_ops: usize, felts: *const u64, n_felts: usize, log_n: c_int, out: *mut *mut mh_trace, results: *mut mh_hash_result, info: *mut mh_hasher_section_info) -> c_int;
    pub fn mh_miden_hasher_section(ctx: *mut mh_ctx, chiplets: *mut mh_trace, ops: *const mh_hash_op, n_ops: usize, felts: *const u64, n_felts: usize, results: *mut mh_hash_result, info: *mut mh_hasher_section_info) -> c_int;
    pub fn mh_hasher_section_tile() -> u32;
    // the bitwise, ACE and kernel-ROM sections and the whole chiplets trace built on the device (csrc/bitwise_section.hip, ace_section.hip,
    // kernel_rom_section.hip, chiplets_build.hip); results, digests and info may be null
    pub fn mh_bitwise_section_build(ctx: *mut mh_ctx, ops: *const mh_bitwise_op, n_ops: usize, log_n: c_int, out: *mut *mut mh_trace, results: *mut u32, info: *mut mh_bitwise_section_info) -> c_int;
    pub fn mh_miden_bitwise_section(ctx: *mut mh_ctx, chiplets: *mut mh_trace, start_row: u64, ops: *const mh_bitwise_op, n_ops: usize, results: *mut u32, info: *mut mh_bitwise_section_info) -> c_int;
    pub fn mh_ace_section_build(ctx: *mut mh_ctx, evals: *const mh_ace_eval, n_evals: usize, felts: *const u64, n_felts: usize, log_n: c_int, out: *mut *mut mh_trace, info: *mut mh_ace_section_info) -> c_int;
    pub fn mh_miden_ace_section(ctx: *mut mh_ctx, chiplets: *mut mh_trace, start_row: u64, evals: *const mh_ace_eval, n_evals: usize, felts: *const u64, n_felts: usize, info: *mut mh_ace_section_info) -> c_int;
    pub fn mh_ace_section_tile() -> u32;
    pub fn mh_kernel_rom_section_build(ctx: *mut mh_ctx, procs: *const u64, n_procs: usize, calls: *const u64, n_calls: usize, log_n: c_int, out: *mut *mut mh_trace, digests: *mut u64, info: *mut mh_kernel_rom_section_info) -> c_int;
    pub fn mh_miden_kernel_rom_section(ctx: *mut mh_ctx, chiplets: *mut mh_trace, start_row: u64, procs: *const u64, n_procs: usize, calls: *const u64, n_calls: usize, digests: *mut u64, info: *mut mh_kernel_rom_section_info) -> c_int;
    pub fn mh_miden_chiplets_build(ctx: *mut mh_ctx, lists: *const mh_chiplets_lists, log_n: c_int, out: *mut *mut mh_trace, info: *mut mh_chiplets_info) -> c_int;
    pub fn mh_miden_chiplets_frame(ctx: *mut mh_ctx, chiplets: *mut mh_trace, padding_start: u64) -> c_int;
    // the precompile prover's Keccak round (width 68) and sponge (width 67) traces built on the device (csrc/keccak_traces.hip); the
    // first two are host only; outputs, digests and info may be null
    pub fn mh_keccak_round_program(out: *mut i32) -> c_int;
    pub fn mh_keccak_round_levels(out: *mut i32) -> c_int;
    pub fn mh_keccak_round_trace_build(ctx: *mut mh_ctx, states: *const u64, n_perms: usize, log_n: c_int, out: *mut *mut mh_trace, outputs: *mut u64) -> c_int;
    pub fn mh_keccak_traces_build(ctx: *mut mh_ctx, bytes: *const u8, n_bytes: usize, msgs: *const mh_keccak_msg, n_msgs: usize, log_round: c_int, log_sponge: c_int, round_out: *mut *mut mh_trace, sponge_out: *mut *mut mh_trace, digests: *mut u8, info: *mut mh_keccak_traces_info) -> c_int;
    pub fn mh_poseidon2_chiplet_plan(abs: *const mh_p2c_absorption, n_abs: usize, refs: *const i64, n_cycles: usize, start: *mut u64, level: *mut u32, info: *mut mh_p2c_info) -> c_int;
    pub fn mh_poseidon2_chiplet_trace_build(ctx: *mut mh_ctx, abs: *const mh_p2c_absorption, n_abs: usize, blocks: *const u64, refs: *const i64, n_cycles: usize, log_n: c_int, out: *mut *mut mh_trace, digests: *mut u64, outputs: *mut u64, info: *mut mh_p2c_info) -> c_int;
    pub fn mh_uint_traces_plan(rows: *const mh_uint_row, n_store: usize, muls: *const mh_uint_mul_op, n_mul: usize, adds: *const mh_uint_add_op, n_add: usize, log_usm: c_int, log_add: c_int, bound_index: *mut u32, info: *mut mh_uint_traces_info) -> c_int;
    pub fn mh_uint_traces_build(ctx: *mut mh_ctx, rows: *const mh_uint_row, n_store: usize, muls: *const mh_uint_mul_op, n_mul: usize, adds: *const mh_uint_add_op, n_add: usize, log_usm: c_int, log_add: c_int, usm_out: *mut *mut mh_trace, add_out: *mut *mut mh_trace, info: *mut mh_uint_traces_info) -> c_int;
    pub fn mh_ec_traces_plan(groups: *const mh_ec_group, n_groups: usize, points: *const mh_ec_point, n_points: usize, adds: *const mh_ec_add_op, n_add: usize, exprs: *const mh_msm_expr, n_exprs: usize, terms: *const mh_msm_term, n_terms: usize, log_groups: c_int, log_points: c_int, log_add: c_int, log_msm: c_int, row_start: *mut u32, info: *mut mh_ec_traces_info) -> c_int;
    pub fn mh_ec_traces_build(ctx: *mut mh_ctx, groups: *const mh_ec_group, n_groups: usize, points: *const mh_ec_point, n_points: usize, adds: *const mh_ec_add_op, n_add: usize, exprs: *const mh_msm_expr, n_exprs: usize, terms: *const mh_msm_term, n_terms: usize, log_groups: c_int, log_points: c_int, log_add: c_int, log_msm: c_int, groups_out: *mut *mut mh_trace, points_out: *mut *mut mh_trace, add_out: *mut *mut mh_trace, msm_out: *mut *mut mh_trace, info: *mut mh_ec_traces_info) -> c_int;
    pub fn mh_chunk_node_plan(bytes: *const u8, n_bytes: usize, digests: *const u8, records: *const mh_kn_record, n: usize, p2_cycles: u64, log_n: c_int, info: *mut mh_chunk_node_info) -> c_int;
    pub fn mh_chunk_node_trace_build(ctx: *mut mh_ctx, p2: *const mh_trace, bytes: *const u8, n_bytes: usize, digests: *const u8, records: *const mh_kn_record, n: usize, log_n: c_int, out: *mut *mut mh_trace, info: *mut mh_chunk_node_info) -> c_int;
    pub fn mh_transcript_eval_plan(nodes: *const mh_te_node, n_nodes: usize, terms: *const mh_te_term, n_terms: usize, limbs: *const u32, n_lit: usize, root: u64, p2_cycles: u64, log_n: c_int, row_start: *mut u32, info: *mut mh_transcript_eval_info) -> c_int;
    pub fn mh_transcript_eval_trace_build(ctx: *mut mh_ctx, p2: *const mh_trace, nodes: *const mh_te_node, n_nodes: usize, terms: *const mh_te_term, n_terms: usize, limbs: *const u32, n_lit: usize, root: u64, log_n: c_int, out: *mut *mut mh_trace, root_felts: *mut u64, info: *mut mh_transcript_eval_info) -> c_int;
}
