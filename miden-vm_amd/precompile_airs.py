"""The second client of the backend: AIRs of the precompile prover (`precompiles-prover/src`), hand-ported against `dag.AirBuilder`
like the VM's three AIRs, and the statement layer of its session (`precompiles-prover/src/session/prove.rs`).

What is here: ALL TWELVE AIRs of `ChipletAir::all()` (session/prove.rs:111-126) -- the HASHING half of the session
(ChunkNode, Poseidon2, KeccakRound, BytePairLut, KeccakSponge; ChunkNode also as its two stand-alone halves), the TRANSCRIPT evaluator
(TranscriptEval), the 256-bit ARITHMETIC (UintStoreMul, UintAdd), and the ELLIPTIC-CURVE half (EcGroups, EcPointStore, EcGroupAdd, EcMsm)
-- and `precompile_session`, a whole deferred-precompile session over them: no stand-in, the transcript root as the public input --
* `BytePairLutAir` (`primitives/byte_pair_lut.rs`): the one AIR of the stack with PREPROCESSED columns and a fixed height -- the
  2^16-row `(a, b, !a & b, a ^ b)` table committed once, three witness multiplicity columns, two LogUp columns;
* `KeccakRoundAir` (`hash/keccak/round/{mod,program}.rs`): its consumer -- a three-address machine `c = ROL(a OP b, s)` whose 128-slot
  round program (ten periodic columns) runs Keccak-f[1600] rounds, two permutation lanes of 34 columns, 2 x 10 LogUp columns (Memory64
  provide / requires, eight byte-pair requests, eight Range16 limb requests per row);
* `EcGroupsAir` (`ec/groups.rs`): six columns, an ungated pointer chain, one LogUp column whose provides are closed by the verifier's
  fixed boundary consumes;
* `ChunkAir` (`hash/chunk/{mod,message,trace}.rs`): the hashers' input tape -- one row per 32-byte chunk, provided as four Memory64
  lanes and absorbed as one Poseidon2 block, twelve columns, FIVE flattened LogUp columns (`frac_col!`) on three buses;
* `Poseidon2Air` (`transcript/poseidon2/{mod,math,program,messages,trace}.rs`): the permutation chiplet that serves those
  absorptions -- the VM's packed 16-row schedule plus thirteen cube registers per row (S-box outputs at degree 3), absorption chains
  and per-cycle In / Out multiplicities; 32 columns, 3 LogUp columns, sixteen periodic columns, log_quotient_degree 2;
* `KeccakSpongeAir` (`hash/keccak/sponge/{mod,program,message,trace}.rs`): pad10*1, absorb and squeeze around the round chiplet's
  permutations -- 67 columns (a padding state machine, lane halves, byte shadows), 24 flattened LogUp columns on Memory64 / the byte-pair
  table / KeccakSponge, eleven periodic columns of period 32, log_quotient_degree 2.  With it a KECCAK-256 HASHING SESSION closes over
  six real chiplets: bytes in (chunk tape), digest out (the round chiplet's output lanes);
* `KeccakNodeAir` (`hash/keccak/node/{mod,trace}.rs`): one row per distinct hashed input -- issues the sponge's request, reads the digest
  lanes, drives the two Poseidon2 permutations of the transcript-DAG node and provides `Binding(H_keccak, True, 0, 0)`; 30 columns, nine
  flattened LogUp columns on six buses.  With it the hashing session runs over SEVEN real chiplets and only the transcript's readers of
  the bindings stay outside;
* `ChunkNodeAir` (`hash/chunk_node/{mod,trace}.rs`): the form `ChipletAir::all()` really runs -- the chunk and the Keccak node chiplets
  side by side on one row range (42 columns, 14 LogUp columns, one sigma); composed here from the same two halves;
* `UintAddAir` (`uint/add/{mod,trace}.rs`): a + b = c (mod p) over stored 256-bit values -- a "vertical Schwartz-Zippel" identity at the
  LogUp challenge beta: the one MAIN constraint of this stack over the extension field that reads a verifier challenge; ternary carries,
  zero-sentinel modes (negation, equality certificate), a nonzero certificate; 30 columns, three LogUp columns, period 2;
* `EcPointStoreAir` (`ec/{mod,trace,require}.rs`): one row per curve point -- its group's five-tuple pulled from `EcGroupsAir`, the
  pointers of x and y, and the membership certificate u = x^2 + a, w = x u + b, y^2 = w as three consumed `UintMul` relations (or the
  point-at-infinity flag, or a closure certificate from the adder); 14 columns, five LogUp columns;
* `EcGroupAddAir` (`ec/add/{mod,trace}.rs`, `ec/require.rs`): R = P + Q for ANY two stored points -- a near-one-hot over five cases whose
  flags ride the consumed `EcPoint` tuples, chord / tangent / tail arithmetic as pointer-level certificates consumed from the uint
  relation chiplets (no limb enters the trace), fresh results minted with closure certificates under a Range16-witnessed pointer
  ordering; 21 columns, twelve LogUp columns on seven buses, four-row blocks;
* `UintStoreMulAir` (`uint/{mod,trace}.rs`, `uint/mul/{mod,trace}.rs`, `uint/store_mul/{mod,trace}.rs`): the range-checked store of the
  256-bit values and the scaled multiply-accumulate relation kappa_a a b +- kappa_c c = r (mod p) side by side on one row range; both
  identities are vertical Schwartz-Zippel checks carried by three extension-field REGISTERS in the aux trace -- the one AIR of the
  session whose `build_aux_trace` computes more than LogUp sums: here the lookup program's register tail, built on the device by a scan
  over affine maps; 44 columns, 26 LogUp columns + 3 registers, 13 periodic columns.  With it the reference's "arithmetic + EC stack"
  runs over SIX real chiplets (BytePairLut, UintStoreMul, UintAdd, EcGroups, EcPointStore, EcGroupAdd) with no stand-in: scalar
  multiples of a curve point, every field operation proven;
* `EcMsmAir` (`ec/msm/{mod,trace,require}.rs`): multi-scalar-multiplication EXPRESSIONS -- runs of (base point, scalar) term rows with a
  value point, built by `intro` / `neg` / `combine` steps the AIR checks one by one (variable-length blocks under an allocator chain,
  merge-walk cursors over the operands' sorted term lists, scalars on a shared base added mod the group order, values added by a consumed
  `EcGroupAdd`, a strict pointer ordering against circular derivations); 38 columns, eleven LogUp columns on nine buses.  SEVEN real
  chiplets prove sum k_i P_i; only the eval chip's resolve of the final expression stays outside;
* `TranscriptEvalAir` (`transcript/eval/{mod,trace}.rs`, `transcript/{binding,nodes}.rs`): the transcript's hasher and binder -- one DAG
  node per row (AND combinators, the ZERO_HASH leaf, uint leaves and pin claims, uint ops, EC create / infinity, EC ops, the multi-row
  EcMsm absorb run), each hashed on the Poseidon2 chiplet under a capacity that names its kind and settled on the `Binding` bus; row 0
  is the root and its hash is the PUBLIC INPUT; 39 columns, sixteen LogUp columns on eleven buses.  With it nothing is left outside:
  `precompile_session` runs the twelve chiplets in the reference's order;
the precompile prover's LogUp adapter (natural last-row sigma closing, `logup/constraint.rs`: `dag.LogUp(closing="sigma_last_row")`),
its bus registry (`relations.rs`) and `ChipletMultiAir::eval_external` (`session/prove.rs:259-272`: sum of the committed sigmas + the
fixed boundary correction).

(Round 6: this module holds the AIR definitions and the statement layer only.  The witness side -- every `*_trace`, the `*Requires`
ledgers, `UintStore`, `EcStore`, the `*_session` builders and the front end described next -- lives in
`miden-vm_amd/testing/precompile_trace.py`, test-only and frozen.)
`Session` / `SessionTraces` (testing/precompile_trace.py) mirror the reference's claim-building front end (session/mod.rs: `keccak`, `pin_uint`, `uint_leaf`, `uint_add` /
`_sub` / `_mul` / `_is`, `ec_create` / `_pai` / `_add` / `_sub` / `_is`, `msm_intro` / `_combine` / `_neg`, `ec_msm`, `assert_and`, `assert_and_fold`,
`finish`) over these ledgers.  Where one of the SMALLER statements needs the other side of a bus that only they touch -- the transcript's readers of the `Binding` tuples in
the hashing session, or, in the smaller sessions of the tests, whatever is left out (`sponge_side_requests`, `chunk_side_requests`,
`keccak_hash_side_requests`, `poseidon2_out_requests`, `binding_requests`, the uint store's `uint_val_requests` and the multiplier's
`uint_mul_requests` -- relations the ledgers check by value when they are recorded) -- it comes from `requirer_air`, a one-interaction-per-row
stand-in written against the same adapter; `eval_external` sums the `EcGroup` part of `fixed_boundary_correction` only (the `UintVal`
part belongs to the uint store).  Pinned: the reference's own unit tests of every ported chiplet replayed (tests/test_precompile_*.py:
programs, layouts, quotient degrees, message encodings, accepting and corrupted traces), FIPS 202 (the round machine against a plain
Keccak-f; keccak256 of the empty input and of "abc" end to end), every bus of every statement balances.  Not pinned (no Rust): the
reference's own evaluation of the same constraints (exported symbolic DAGs, tools/ref_fixtures), and the quotient degree its symbolic
builder assigns to the Keccak ROUND chiplet (this builder counts a periodic value as degree 1: log_quotient_degree 2, the reference's
notes say 1; for the chunk, Poseidon2, sponge and node chiplets the reference's tests assert 1 / 2 / 2 / 1 and this builder gives the same).
Parity of the device path is held by tests/test_gpu_precompile.py."""
import numpy as np
from . import dag

P = dag.P

# relations.rs:52-80 (bus ids), :91 (MAX_MESSAGE_WIDTH), :78 (NUM_BUS_IDS); logup/mod.rs:103 (NUM_RANDOMNESS), :131 (NUM_PUBLIC_VALUES),
# :146 (NUM_SIGMA_VALUES)
BUS_BYTE_PAIR_LUT, BUS_RANGE16, BUS_MEMORY64, BUS_KECCAK_SPONGE, BUS_EC_GROUP = 0, 1, 4, 5, 14
BUS_POSEIDON2_IN, BUS_POSEIDON2_OUT, BUS_BINDING, BUS_CHUNK_CHAIN, BUS_UINT_VAL, BUS_UINT_ADD = 6, 7, 8, 9, 10, 11
MAX_MESSAGE_WIDTH, NUM_BUS_IDS = 18, 21
NUM_RANDOMNESS, NUM_PUBLIC_VALUES, NUM_SIGMA_VALUES = 2, 4, 1
PLACEHOLDER_RELATION_DIGEST = (0, 0, 0, 0)  # session/prove.rs:40

# primitives/byte_pair_lut.rs:56-80, :96-130
OP_ANDNOT, OP_XOR = 0, 1
BPL_TRACE_HEIGHT = 1 << 16
BPL_MAIN_COLS, BPL_AUX_COLS, BPL_PREP_COLS = 3, 2, 4

# precompiles/src/math/curve/mod.rs:57-62, precompiles/src/math/uint/domain.rs:9-13: the fixed environment (session/fixed.rs)
K1_GROUP_PTR, K1_A_PTR, K1_B_PTR, U256_BOUND_PTR, K1_BASE_BOUND_PTR, K1_SCALAR_BOUND_PTR = 1, 8, 9, 1, 2, 3
FIXED_EC_GROUPS = [(K1_GROUP_PTR, K1_A_PTR, K1_B_PTR, K1_BASE_BOUND_PTR, K1_SCALAR_BOUND_PTR)]  # fixed_ecgroup_msgs, CurveId::ALL
# `fixed_uints` (session/fixed.rs:15-31): (ptr, bound_ptr, value) -- the three domain bounds (moduli rows: their own bound; U256's is 2^256 - 1,
# precompiles/src/math/{u256,k1_base,k1_scalar}.rs `minus_one`), then secp256k1's coefficients under the base-field bound
FIXED_UINTS = [(U256_BOUND_PTR, U256_BOUND_PTR, (1 << 256) - 1),
               (K1_BASE_BOUND_PTR, K1_BASE_BOUND_PTR, 0xFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFEFFFFFC2E),
               (K1_SCALAR_BOUND_PTR, K1_SCALAR_BOUND_PTR, 0xFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFEBAAEDCE6AF48A03BBFD25E8CD0364140),
               (K1_A_PTR, K1_BASE_BOUND_PTR, 0), (K1_B_PTR, K1_BASE_BOUND_PTR, 7)]


def _host_aux(air_lookup, host_aux, preprocessed=None):
    if host_aux is None:
        return None

    def build_aux(main, randomness):
        aux, fin = host_aux(air_lookup, main, randomness, preprocessed)
        return aux, [int(fin[0]), int(fin[1])]
    return build_aux


# ---- BytePairLut ---------------------------------------------------------------------------------------------------------------------
def byte_pair_preprocessed():
    """`preprocessed_table` (byte_pair_lut.rs:262-277): every (a, b) in lex order, idx = a << 8 | b, with !a & b and a ^ b."""
    idx = np.arange(BPL_TRACE_HEIGHT, dtype=np.uint64)
    a, b = idx >> np.uint64(8), idx & np.uint64(0xff)
    return np.stack([a, b, (~a & np.uint64(0xff)) & b, a ^ b], axis=1).astype(np.uint64)


def byte_pair_lut_air(host_aux=None):
    """-> (dag.Air with `.preprocessed`, dag.Lookup).  `BytePairLutAir::eval` (byte_pair_lut.rs:421-432: no local constraints) and its
    `LookupAir::eval` (:463-528): column 0 = the AndNot self-provide, column 1 = the Xor and Range16 self-provides; the lookup reads
    the combined `[preprocessed ++ main]` window."""
    b = dag.AirBuilder(BPL_MAIN_COLS, aux_width=BPL_AUX_COLS, num_randomness=NUM_RANDOMNESS, num_aux_values=NUM_SIGMA_VALUES,
                       num_public=NUM_PUBLIC_VALUES, preprocessed_width=BPL_PREP_COLS)
    lk = dag.LogUp(b, MAX_MESSAGE_WIDTH, NUM_BUS_IDS, closing="sigma_last_row")

    def side(bb):
        a, bv, c_andnot, c_xor = (bb.preprocessed(i) for i in range(4))
        neg = [bb.const(0) - bb.main(i) for i in range(3)]  # provides: negative multiplicities
        return dict(a=a, b=bv, c_andnot=c_andnot, c_xor=c_xor, w=a + bb.const(256) * bv, neg=neg, one=bb.const(1),
                    andnot=bb.const(OP_ANDNOT), xor=bb.const(OP_XOR))
    sc, sp = side(lk.b), side(lk.lb)

    def msg(f):  # a message written once: f(side) -> (bus, fields), encoded with whichever Challenges it is given
        def m(ch):
            bus, fields = f(sc if ch is lk.ch_c else sp)
            return ch.encode(bus, fields)
        return m
    one = (sc["one"], sp["one"])
    with lk.column() as col:  # frac_col!: one group, one batch with flag ONE (logup/mod.rs:70-84)
        with col.group() as g:
            with g.batch(one) as bt:
                bt.insert((sc["neg"][0], sp["neg"][0]), msg(lambda s: (BUS_BYTE_PAIR_LUT, [s["andnot"], s["a"], s["b"], s["c_andnot"]])))
    with lk.column() as col:
        with col.group() as g:
            with g.batch(one) as bt:
                bt.insert((sc["neg"][1], sp["neg"][1]), msg(lambda s: (BUS_BYTE_PAIR_LUT, [s["xor"], s["a"], s["b"], s["c_xor"]])))
                bt.insert((sc["neg"][2], sp["neg"][2]), msg(lambda s: (BUS_RANGE16, [s["w"]])))
    lookup = lk.finish("byte_pair_lut")
    assert b.max_degree <= 3, b.max_degree  # "every closing constraint stays at degree <= 3 -> lqd 1"
    prep = byte_pair_preprocessed()
    return dag.Air(b, _host_aux(lookup, host_aux, prep), "byte_pair_lut", preprocessed=prep), lookup


# mh_fill_multiplicities: the table's three multiplicity columns (the per-pair ledger of byte_pair_lut.rs:134-226, filled from the
# consumers' pushes on the device) as (lookup_column, fraction, main_column); the instance is the chiplet's index in the session
BYTE_PAIR_LUT_MULT_SLOTS = [(0, 0, 0), (1, 0, 1), (1, 1, 2)]


# ---- EcGroups ------------------------------------------------------------------------------------------------------------------------
EC_GROUPS_COLS = 6  # ptr, a_ptr, b_ptr, bound_ptr, scalar_bound_ptr, mult (ec/groups.rs:59-74)


def ec_groups_air(host_aux=None):
    """`EcGroupsAir::eval` (ec/groups.rs:120-139: `ptr' = ptr + 1` on transitions, `ptr = 1` on the first row) and its one LogUp
    column (:163-202): the `EcGroup` provide at multiplicity `-mult`."""
    b = dag.AirBuilder(EC_GROUPS_COLS, aux_width=1, num_randomness=NUM_RANDOMNESS, num_aux_values=NUM_SIGMA_VALUES,
                       num_public=NUM_PUBLIC_VALUES)
    b.assert_zero(b.is_transition() * (b.main(0, 1) - b.main(0) - b.const(1)))
    b.assert_zero(b.is_first_row() * (b.main(0) - b.const(1)))
    lk = dag.LogUp(b, MAX_MESSAGE_WIDTH, NUM_BUS_IDS, closing="sigma_last_row")

    def msg(ch):
        bb = lk.b if ch is lk.ch_c else lk.lb
        return ch.encode(BUS_EC_GROUP, [bb.main(i) for i in range(5)])
    with lk.column() as col:
        with col.group() as g:
            with g.batch((lk.b.const(1), lk.lb.const(1))) as bt:
                bt.insert((lk.b.const(0) - lk.b.main(5), lk.lb.const(0) - lk.lb.main(5)), msg)
    lookup = lk.finish("ec_groups")
    return dag.Air(b, _host_aux(lookup, host_aux), "ec_groups"), lookup


# ---- the requests of chiplets a statement leaves out ---------------------------------------------------------------------------------
REQUIRER_COLS = 2 + 4  # multiplicity | bus id + 1 | up to four payload felts


def requirer_air(host_aux=None, payload=4):
    """A stand-in for the consumers of the byte-pair table (the Keccak round chiplet's byte and limb requests,
    hash/keccak/round/mod.rs:396-560): one interaction per row, multiplicity `m` on `bus_prefix[bus] + <beta^i, f_i>` with the bus id
    as a column (the prefix is linear in it, logup/mod.rs:44-47), through the same sigma-closing adapter.  `payload` = the number of
    payload columns (4: the byte-pair / Memory64 shapes; 6: Poseidon2In's `(perm_seq_id, tag, c0..c3)`)."""
    b = dag.AirBuilder(2 + payload, aux_width=1, num_randomness=NUM_RANDOMNESS, num_aux_values=NUM_SIGMA_VALUES,
                       num_public=NUM_PUBLIC_VALUES)
    lk = dag.LogUp(b, MAX_MESSAGE_WIDTH, NUM_BUS_IDS, closing="sigma_last_row")

    def msg(ch):
        bb = lk.b if ch is lk.ch_c else lk.lb
        gamma = ch.bus_prefix[1] - ch.bus_prefix[0]
        acc = ch.alpha + gamma * bb.main(1)
        for i in range(payload):
            acc = acc + ch.beta_powers[i] * bb.main(2 + i)
        return acc
    with lk.column() as col:
        with col.group() as g:
            with g.batch((lk.b.const(1), lk.lb.const(1))) as bt:
                bt.insert((lk.b.main(0), lk.lb.main(0)), msg)
    name = "requirer" if payload == 4 else f"requirer{payload}"
    lookup = lk.finish(name)
    return dag.Air(b, _host_aux(lookup, host_aux), name), lookup


# ---- the statement: ChipletMultiAir (session/prove.rs:222-272) restricted to the ported AIRs -----------------------------------------
def _e_mul(a, b):
    return ((a[0] * b[0] + 7 * a[1] * b[1]) % P, (a[0] * b[1] + a[1] * b[0]) % P)


def _e_inv(a):
    n = (a[0] * a[0] - 7 * a[1] * a[1]) % P
    ni = pow(n, P - 2, P)
    return (a[0] * ni % P, (P - a[1]) * ni % P)


def _encode(alpha, beta, bus, fields):
    """`Challenges::encode` on field values: bus_prefix[bus] + sum beta^i f_i, bus_prefix = alpha + (bus + 1) beta^W."""
    pw, acc = (1, 0), (0, 0)
    for i in range(MAX_MESSAGE_WIDTH):
        if i < len(fields):
            acc = ((acc[0] + pw[0] * fields[i]) % P, (acc[1] + pw[1] * fields[i]) % P)
        pw = _e_mul(pw, beta)
    return ((alpha[0] + (bus + 1) * pw[0] + acc[0]) % P, (alpha[1] + (bus + 1) * pw[1] + acc[1]) % P)


def eval_external(randomness, aux_values, fixed_uints=False):
    """`ChipletMultiAir::eval_external` (session/prove.rs:243-256): sigma_sum(aux_values) + fixed_boundary_correction(challenges) (:205-216)
    -- the verifier's `EcGroup` consumes of the fixed curve groups and, with `fixed_uints` (statements that run the real uint store with
    the fixed environment installed), its `UintVal` consumes of the five fixed uints (session/fixed.rs).  randomness = [alpha, beta] as
    (c0, c1) pairs; aux_values[i] = AIR i's committed values (one sigma each).  -> [one EF value that must vanish]."""
    alpha, beta = randomness[0], randomness[1]
    s = (0, 0)
    for av in aux_values:
        s = ((s[0] + av[0][0]) % P, (s[1] + av[0][1]) % P)
    msgs = [(BUS_EC_GROUP, list(g)) for g in FIXED_EC_GROUPS]
    if fixed_uints:
        msgs += [(BUS_UINT_VAL, [ptr, bound_ptr] + [(v >> (32 * j)) & 0xffffffff for j in range(8)]) for ptr, bound_ptr, v in FIXED_UINTS]
    for bus, fields in msgs:
        inv = _e_inv(_encode(alpha, beta, bus, fields))
        s = ((s[0] + inv[0]) % P, (s[1] + inv[1]) % P)
    return [s]


def external_assertions(pkg, fixed_uints=False):
    return pkg.external_callback(lambda rnd, aux_values, lhs: eval_external(rnd, aux_values, fixed_uints))


# ---- Chunk: the input-byte tape of the hashers (hash/chunk/{mod,message,trace}.rs) ------------------------------------------------------
# One row per 32-byte chunk = 8 u32 felts = four Memory64 lanes for the downstream hasher AND one Poseidon2 absorption block
# (`rate0 || rate1`) of the chain that content-hashes the invocation; chain heads also consume the capacity `Tag::CHUNKS` and
# provide a `ChunkChain` tuple tying the chunk-side index to the P2 chain.  12 main columns, FIVE flattened LogUp columns
# (`frac_col!`, logup/mod.rs:13-28: one column = one group = one batch under the flag ONE), no periodic columns.
CHUNK_COLS, CHUNK_AUX_COLS, CHUNK_NUM_F = 12, 5, 8                      # chunk/mod.rs:55-83, :96
COL_CHUNK_SEQ_ID, COL_PERM_SEQ_ID, COL_CHUNK_ACT, COL_IS_HEAD, COL_F_BEGIN = 0, 1, 2, 3, 4
CHUNK_ADDR_BASE = 1 << 48                                               # hash/memory64.rs:40
TAG_CHUNKS_WORD = (2, 0, 0, 0)                                          # Tag::CHUNKS.as_word(), core/src/deferred/node.rs:47-56, :91-93
POSEIDON2_IN_TAG_RATE0, POSEIDON2_IN_TAG_RATE1, POSEIDON2_IN_TAG_CAP = 0, 1, 2   # transcript/poseidon2/messages.rs:19-23


def _chunk_local(b, off=0):
    """The local constraints of `ChunkAir::eval` (hash/chunk/mod.rs:149-200) over the main columns [off, off + 12)."""
    loc, nxt = [b.main(off + c) for c in range(CHUNK_COLS)], [b.main(off + c, 1) for c in range(CHUNK_COLS)]
    one = b.const(1)
    chunk_seq_id, chunk_seq_id_next = loc[COL_CHUNK_SEQ_ID], nxt[COL_CHUNK_SEQ_ID]
    perm_seq_id, perm_seq_id_next = loc[COL_PERM_SEQ_ID], nxt[COL_PERM_SEQ_ID]
    act, act_next, is_head, is_head_next = loc[COL_CHUNK_ACT], nxt[COL_CHUNK_ACT], loc[COL_IS_HEAD], nxt[COL_IS_HEAD]
    b.assert_zero(b.is_first_row() * chunk_seq_id)
    b.assert_zero(b.is_transition() * (chunk_seq_id_next - chunk_seq_id - one))
    b.assert_zero(b.is_transition() * ((one - is_head_next) * (perm_seq_id_next - perm_seq_id - one)))
    b.assert_zero((one - act) * act)                                    # assert_bool(act)
    b.assert_zero(b.is_transition() * ((one - act) * act_next))
    b.assert_zero((one - is_head) * is_head)                            # assert_bool(is_head)
    b.assert_zero(is_head * (one - act))


def _chunk_columns(lk, off=0):
    """The five flattened LogUp columns of `ChunkAir` (hash/chunk/mod.rs:223-360) -> [[(multiplicity pair, message)]]."""
    def side(ch):
        bb = lk.b if ch is lk.ch_c else lk.lb
        row = [bb.main(off + c) for c in range(CHUNK_COLS)]
        return bb, row, row[COL_F_BEGIN:COL_F_BEGIN + CHUNK_NUM_F]

    def lane(j):        # Memory64Msg { addr: CHUNK_ADDR_BASE + 4 chunk_seq_id + j, lo: f[2j], hi: f[2j + 1] } (hash/memory64.rs:55-64)
        def msg(ch):
            bb, row, f = side(ch)
            addr = bb.const(CHUNK_ADDR_BASE) + bb.const(4) * row[COL_CHUNK_SEQ_ID]
            if j:
                addr = addr + bb.const(j)
            return ch.encode(BUS_MEMORY64, [addr, f[2 * j], f[2 * j + 1]])
        return msg

    def p2_in(tag, which):   # Poseidon2InMsg::{rate0, rate1, cap} (transcript/poseidon2/messages.rs:43-87)
        def msg(ch):
            bb, row, f = side(ch)
            c = [bb.const(x) for x in TAG_CHUNKS_WORD] if which is None else f[4 * which:4 * which + 4]
            return ch.encode(BUS_POSEIDON2_IN, [row[COL_PERM_SEQ_ID], bb.const(tag)] + c)
        return msg

    def emit(ch):            # ChunkChainMsg (hash/chunk/message.rs)
        _, row, _ = side(ch)
        return ch.encode(BUS_CHUNK_CHAIN, [row[COL_CHUNK_SEQ_ID], row[COL_PERM_SEQ_ID]])

    def mults(fn):
        return fn(lk.b), fn(lk.lb)
    neg_act = mults(lambda bb: bb.const(0) - bb.main(off + COL_CHUNK_ACT))
    pos_act = mults(lambda bb: bb.main(off + COL_CHUNK_ACT))
    pos_act_head = mults(lambda bb: bb.main(off + COL_CHUNK_ACT) * bb.main(off + COL_IS_HEAD))
    neg_act_head = mults(lambda bb: bb.const(0) - bb.main(off + COL_CHUNK_ACT) * bb.main(off + COL_IS_HEAD))
    return [[(neg_act, lane(0))], [(neg_act, lane(1)), (neg_act, lane(2))], [(neg_act, lane(3)), (pos_act, p2_in(POSEIDON2_IN_TAG_RATE0, 0))],
            [(pos_act, p2_in(POSEIDON2_IN_TAG_RATE1, 1)), (pos_act_head, p2_in(POSEIDON2_IN_TAG_CAP, None))], [(neg_act_head, emit)]]


def _emit_frac_cols(lk, columns):
    """`frac_col!` (logup/mod.rs:13-28) per entry: one column = one group = one batch of its fractions under the flag ONE."""
    for fractions in columns:
        with lk.column() as col:
            with col.group() as g:
                with g.batch((lk.b.const(1), lk.lb.const(1))) as bt:
                    for mult, msg in fractions:
                        bt.insert(mult, msg)


def chunk_air(host_aux=None):
    """`ChunkAir::eval` (hash/chunk/mod.rs:149-200): `chunk_seq_id` = the row index, `perm_seq_id` + 1 inside a chain and free at chain
    heads, `act` sticky downward, `is_head` boolean and dead on inactive rows; and its `LookupAir::eval` (:223-360): col 0 lane0 |
    col 1 lane1 + lane2 | col 2 lane3 + rate0 | col 3 rate1 + cap | col 4 the ChunkChain emit."""
    b = dag.AirBuilder(CHUNK_COLS, aux_width=CHUNK_AUX_COLS, num_randomness=NUM_RANDOMNESS, num_aux_values=NUM_SIGMA_VALUES,
                       num_public=NUM_PUBLIC_VALUES)
    _chunk_local(b)
    lk = dag.LogUp(b, MAX_MESSAGE_WIDTH, NUM_BUS_IDS, closing="sigma_last_row")
    _emit_frac_cols(lk, _chunk_columns(lk))
    lookup = lk.finish("chunk")
    return dag.Air(b, _host_aux(lookup, host_aux), "chunk"), lookup


# ---- Poseidon2: the permutation chiplet of the transcript (transcript/poseidon2/{mod,math,program,messages,trace}.rs) --------------------
# One 16-row cycle per permutation on the VM's packed schedule (row 0 init + ext, 1-3 ext, 4-10 three internal rounds per row with
# witnessed S-box outputs, 11 int + ext, 12-14 ext, 15 the output), the SAME sixteen periodic columns as the VM's
# Poseidon2PermutationAir.  What it adds: thirteen CUBE REGISTERS per row (x^3 of every S-box input committed, so an S-box output is
# reg^2 x: degree 3 instead of 7 at the price of a degree-3 check reg - x^3), absorption CHAINS (`is_absorb`: the cycle inherits its
# capacity from the previous cycle's output), and per-cycle provide multiplicities for the In side (rate0, rate1, capacity) and the
# Out side (the digest of a chain's last cycle).  32 main columns, 3 LogUp columns, log_quotient_degree 2.
P2_COLS, P2_AUX_COLS, P2_NUM_WITNESSES, P2_NUM_CUBE_REGS, P2_PERIOD = 32, 3, 3, 13, 16      # mod.rs:64-97, math.rs:11-13, program.rs:6
P2C_PERM_SEQ_ID, P2C_IN_MULT, P2C_OUT_MULT, P2C_IS_ABSORB, P2C_STATE, P2C_WITNESS, P2C_CUBE = 0, 1, 2, 3, 4, 16, 19


def _p2_sbox(x, reg):      # math.rs `sbox`: (reg^2 x, reg - x^3)
    return reg * reg * x, reg - (x * x) * x


def poseidon2_chiplet_air(host_aux=None):
    """`Poseidon2Air::eval` (transcript/poseidon2/mod.rs:176-345) over the round functions of math.rs, and its `LookupAir::eval`
    (:368-516): col 0 in_rate0 | col 1 in_rate1 + out_rate0 | col 2 in_cap."""
    from . import miden_air as MA
    b = dag.AirBuilder(P2_COLS, aux_width=P2_AUX_COLS, num_randomness=NUM_RANDOMNESS, num_aux_values=NUM_SIGMA_VALUES,
                       num_public=NUM_PUBLIC_VALUES, periodic=MA.periodic_columns())
    loc, nxt = [b.main(c) for c in range(P2_COLS)], [b.main(c, 1) for c in range(P2_COLS)]
    one = b.const(1)
    per = [b.periodic_value(i) for i in range(16)]
    is_init_ext, is_ext, is_packed_int, is_int_ext = per[0:4]
    ark = per[4:16]
    p_last = one - is_init_ext - is_ext - is_packed_int - is_int_ext
    state, state_next = loc[P2C_STATE:P2C_STATE + 12], nxt[P2C_STATE:P2C_STATE + 12]
    w, regs = loc[P2C_WITNESS:P2C_WITNESS + 3], loc[P2C_CUBE:P2C_CUBE + P2_NUM_CUBE_REGS]
    perm_seq_id, perm_seq_id_next = loc[P2C_PERM_SEQ_ID], nxt[P2C_PERM_SEQ_ID]
    in_mult, in_mult_next, out_mult, out_mult_next = loc[P2C_IN_MULT], nxt[P2C_IN_MULT], loc[P2C_OUT_MULT], nxt[P2C_OUT_MULT]
    is_absorb, is_absorb_next = loc[P2C_IS_ABSORB], nxt[P2C_IS_ABSORB]
    activity = in_mult + out_mult
    b.assert_zero(b.is_first_row() * perm_seq_id)
    b.assert_zero(b.is_first_row() * is_absorb)
    b.assert_zero((one - p_last) * (perm_seq_id_next - perm_seq_id))
    b.assert_zero(b.is_transition() * (p_last * (perm_seq_id_next - perm_seq_id - one)))
    b.assert_zero((one - p_last) * (in_mult_next - in_mult))
    b.assert_zero((one - p_last) * (out_mult_next - out_mult))
    b.assert_zero((one - is_absorb) * is_absorb)
    b.assert_zero((one - p_last) * (is_absorb_next - is_absorb))
    for i in range(8, 12):
        b.assert_zero(p_last * is_absorb_next * (state_next[i] - state[i]))
    diag = [b.const(v) for v in MA.MAT_DIAG]

    def ext_with_cubes(inputs):
        outs, checks = [], []
        for i in range(12):
            o, c = _p2_sbox(inputs[i], regs[i])
            outs.append(o)
            checks.append(c)
        return MA._matmul_external(outs), checks

    def emit(gate, next_state, checks_first, checks_after=()):
        for c in checks_first:
            b.assert_zero(gate * c)
        for i in range(12):
            b.assert_zero(gate * (state_next[i] - next_state[i]))
        for c in checks_after:
            b.assert_zero(gate * c)
    # row 0: apply_init_plus_ext -- next-state constraints first, then the cube checks (mod.rs:262-272)
    pre = MA._matmul_external(state)
    expected, cubes = ext_with_cubes([pre[i] + ark[i] for i in range(12)])
    emit(activity * is_init_ext, expected, (), cubes)
    # rows 1-3, 12-14: apply_single_ext
    expected, cubes = ext_with_cubes([state[i] + ark[i] for i in range(12)])
    emit(activity * is_ext, expected, (), cubes)
    # rows 4-10: apply_packed_internals -- witness checks, cube checks, next state
    st, wit_checks, cube_checks = list(state), [], []
    for k in range(3):
        out, chk = _p2_sbox(st[0] + ark[k], regs[k])
        wit_checks.append(w[k] - out)
        cube_checks.append(chk)
        st[0] = w[k]
        st = MA._matmul_internal(st, diag)
    emit(activity * is_packed_int, st, wit_checks + cube_checks)
    # row 11: apply_internal_plus_ext -- the witness check, the cube checks (the internal one first), next state
    int_out, int_chk = _p2_sbox(state[0] + b.const(MA.ARK_INT[MA.LAST_INTERNAL_ROUND_ARK_IDX]), regs[12])
    inter = MA._matmul_internal([w[0]] + state[1:], diag)
    expected, cubes = ext_with_cubes([inter[i] + ark[i] for i in range(12)])
    emit(activity * is_int_ext, expected, [w[0] - int_out, int_chk] + cubes)
    b.assert_zero((one - is_packed_int - is_int_ext) * w[0])
    b.assert_zero((one - is_packed_int) * w[1])
    b.assert_zero((one - is_packed_int) * w[2])

    lk = dag.LogUp(b, MAX_MESSAGE_WIDTH, NUM_BUS_IDS, closing="sigma_last_row")

    def side(ch):
        bb = lk.b if ch is lk.ch_c else lk.lb
        return bb, [bb.main(c) for c in range(P2_COLS)]

    def p2_in(tag, lo):
        def msg(ch):
            bb, row = side(ch)
            return ch.encode(BUS_POSEIDON2_IN, [row[P2C_PERM_SEQ_ID], bb.const(tag)] + row[P2C_STATE + lo:P2C_STATE + lo + 4])
        return msg

    def p2_out(ch):
        _, row = side(ch)
        return ch.encode(BUS_POSEIDON2_OUT, [row[P2C_PERM_SEQ_ID]] + row[P2C_STATE:P2C_STATE + 4])

    def mults(fn):
        return fn(lk.b), fn(lk.lb)

    def sel(bb):
        pv = [bb.periodic_value(i) for i in range(4)]
        return pv[0], bb.const(1) - pv[0] - pv[1] - pv[2] - pv[3]
    m_in = mults(lambda bb: sel(bb)[0] * (bb.const(0) - bb.main(P2C_IN_MULT)))
    m_in_cap = mults(lambda bb: sel(bb)[0] * ((bb.const(0) - bb.main(P2C_IN_MULT)) * (bb.const(1) - bb.main(P2C_IS_ABSORB))))
    m_out = mults(lambda bb: sel(bb)[1] * ((bb.const(0) - bb.main(P2C_OUT_MULT)) * (bb.const(1) - bb.main(P2C_IS_ABSORB, 1))))
    for fractions in ([(m_in, p2_in(POSEIDON2_IN_TAG_RATE0, 0))], [(m_in, p2_in(POSEIDON2_IN_TAG_RATE1, 4)), (m_out, p2_out)],
                      [(m_in_cap, p2_in(POSEIDON2_IN_TAG_CAP, 8))]):
        with lk.column() as col:
            with col.group() as g:
                with g.batch((lk.b.const(1), lk.lb.const(1))) as bt:
                    for mult, msg in fractions:
                        bt.insert(mult, msg)
    lookup = lk.finish("poseidon2_chiplet")
    return dag.Air(b, _host_aux(lookup, host_aux), "poseidon2_chiplet"), lookup


# ---- KeccakRound: the consumer of the byte-pair table (hash/keccak/round/{mod,program}.rs) --------------------------------------------
# A three-address machine `c = ROL(a OP b, s)` over the Memory64 bus; one Keccak-f[1600] round = 128 program slots (10 periodic
# columns), a permutation = 24 active rounds + 1 dead round = 3200 rows, two permutation lanes side by side (2 x 34 main columns,
# 2 x 10 LogUp columns).  Every row commits its operands and result as bytes / 16-bit limbs and checks them against the table.
ROUND_PERIOD, KR_NUM_ROUNDS, KR_NUM_LANES, KR_LANE_WIDTH = 128, 24, 2, 34
PERM_CYCLE = (KR_NUM_ROUNDS + 1) * ROUND_PERIOD
KR_MAIN_COLS, KR_AUX_COLS, KR_IP_BOUNDARY = KR_LANE_WIDTH * KR_NUM_LANES, 10 * KR_NUM_LANES, 25
KR_COL_IP, KR_A, KR_B, KR_R, KR_ROT, KR_COL_ACT = 0, 1, 9, 17, 25, 33  # lane-local (mod.rs:52-96)
PCOL_IS_XOR, PCOL_IS_ANDNOT, PCOL_IS_ROL, PCOL_BACK_A, PCOL_BACK_B, PCOL_K, PCOL_DST_MULT, PCOL_P_LAST, PCOL_IS_XORROL, PCOL_SWAP = range(10)
OP_NOP, OP_KXOR, OP_KANDNOT, OP_ROL, OP_XORROL = range(5)
KECCAK_RC = [0x0000000000000001, 0x0000000000008082, 0x800000000000808a, 0x8000000080008000, 0x000000000000808b, 0x0000000080000001,
             0x8000000080008081, 0x8000000000008009, 0x000000000000008a, 0x0000000000000088, 0x0000000080008009, 0x000000008000000a,
             0x000000008000808b, 0x800000000000008b, 0x8000000000008089, 0x8000000000008003, 0x8000000000008002, 0x8000000000000080,
             0x000000000000800a, 0x800000008000000a, 0x8000000080008081, 0x8000000000008080, 0x0000000080000001, 0x8000000080008008]
KECCAK_RHO = [[0, 36, 3, 41, 18], [1, 44, 10, 45, 2], [62, 6, 43, 15, 61], [28, 55, 25, 21, 56], [27, 20, 39, 8, 14]]  # RHO[x][y]
SLOT_RC, SLOT_C_BEGIN, SLOT_D_ROL_BEGIN, SLOT_D_XOR_BEGIN, SLOT_CHI_ANDNOT_BEGIN, SLOT_CHI00, SLOT_IOTA, SLOT_CHI_XOR_BEGIN = 0, 2, 22, 27, 69, 102, 103, 104
_SLOT_B = [32, 34, 36, 37, 38, 39, 40, 41, 43, 46, 47, 48, 49, 50, 51, 52, 54, 55, 56, 58, 61, 63, 65, 67, 68]  # program.rs:165-194
M64 = (1 << 64) - 1


def keccak_round_slots():
    """`slots()` (program.rs:262-270): per slot (op, shift, back_a, back_b, dst_mult).  Sources are ("local", slot) /
    ("lane", x, y) = the previous round's output for lane (x, y) / None, turned into back-offsets exactly as `Source::back_off`."""
    def slot_lane_prev(x, y):
        return SLOT_IOTA if (x, y) == (0, 0) else SLOT_CHI_XOR_BEGIN + (x + 5 * y - 1)

    def slot_c(x):
        return SLOT_C_BEGIN + 4 * x + 3

    def slot_t(x, y):
        return SLOT_CHI_ANDNOT_BEGIN + x + 5 * y

    def slot_b(x, y):
        return _SLOT_B[x + 5 * y]
    s = [(OP_NOP, 0, None, None, 0)] * ROUND_PERIOD
    for x in range(5):  # theta C: five linear 4-XOR chains
        base = SLOT_C_BEGIN + 4 * x
        s[base] = (OP_KXOR, 0, ("lane", x, 0), ("lane", x, 1), 1)
        s[base + 1] = (OP_KXOR, 0, ("local", base), ("lane", x, 2), 1)
        s[base + 2] = (OP_KXOR, 0, ("local", base + 1), ("lane", x, 3), 1)
        s[base + 3] = (OP_KXOR, 0, ("local", base + 2), ("lane", x, 4), 2)
    for i in range(5):
        s[SLOT_D_ROL_BEGIN + i] = (OP_ROL, 1, ("local", slot_c((i + 1) % 5)), None, 1)
    for i in range(5):
        s[SLOT_D_XOR_BEGIN + i] = (OP_KXOR, 0, ("local", slot_c((i + 4) % 5)), ("local", SLOT_D_ROL_BEGIN + i), 5)
    for out_y in range(5):  # theta-apply + rho-pi, `emit_apply_rpi`
        for out_x in range(5):
            in_x, in_y = (3 * out_y + out_x) % 5, out_x  # pi^-1
            rho = KECCAK_RHO[in_x][in_y]
            a_src, d_src = ("lane", in_x, in_y), ("local", SLOT_D_XOR_BEGIN + in_x)
            apply_a, apply_b = (d_src, a_src) if in_y == 0 else (a_src, d_src)
            s[slot_b(out_x, out_y)] = (OP_KXOR if rho == 0 else OP_XORROL, rho, apply_a, apply_b, 3)
    for y in range(5):
        for x in range(5):
            s[slot_t(x, y)] = (OP_KANDNOT, 0, ("local", slot_b((x + 1) % 5, y)), ("local", slot_b((x + 2) % 5, y)), 1)
    s[SLOT_CHI00] = (OP_KXOR, 0, ("local", slot_t(0, 0)), ("local", slot_b(0, 0)), 1)
    s[SLOT_IOTA] = (OP_KXOR, 0, ("local", SLOT_CHI00), ("local", SLOT_RC), 2)
    for idx in range(1, 25):
        x, y = idx % 5, idx // 5
        s[SLOT_CHI_XOR_BEGIN + idx - 1] = (OP_KXOR, 0, ("local", slot_t(x, y)), ("local", slot_b(x, y)), 2)

    def back(src, read_slot):
        if src is None:
            return 0
        if src[0] == "local":
            return read_slot - src[1]
        return ROUND_PERIOD + read_slot - slot_lane_prev(src[1], src[2])
    return [(op, sh, back(a, i), back(bsrc, i), m) for i, (op, sh, a, bsrc, m) in enumerate(s)]


def _rol_decompose(s):  # program.rs:470-472
    return (s - 32, 1) if s >= 32 else (s, 0)


def keccak_round_program():
    """`round_program()` (program.rs:481-519): the ten period-128 columns in PCOL_* order."""
    cols = [[0] * ROUND_PERIOD for _ in range(10)]
    for slot, (op, sh, back_a, back_b, mult) in enumerate(keccak_round_slots()):
        is_xor, is_andnot, is_rol, is_xorrol, k, swap = {OP_NOP: (0, 0, 0, 0, 0, 0), OP_KXOR: (1, 0, 0, 0, 0, 0), OP_KANDNOT: (0, 1, 0, 0, 0, 0)}.get(op, None) or \
            ((0, 0, 1, 0, 1 << sh, 0) if op == OP_ROL else (1, 0, 1, 1, 1 << _rol_decompose(sh)[0], _rol_decompose(sh)[1]))
        for c, v in ((PCOL_IS_XOR, is_xor), (PCOL_IS_ANDNOT, is_andnot), (PCOL_IS_ROL, is_rol), (PCOL_IS_XORROL, is_xorrol), (PCOL_SWAP, swap),
                     (PCOL_BACK_A, back_a), (PCOL_BACK_B, back_b), (PCOL_K, k), (PCOL_DST_MULT, mult)):
            cols[c][slot] = v
    cols[PCOL_P_LAST][ROUND_PERIOD - 1] = 1
    return cols


def _pack_le(items, base):  # utils.rs `pack_le`: Horner, LSB first
    acc = None
    for it in reversed(items):
        acc = it if acc is None else acc * base + it
    return acc


def keccak_round_air(host_aux=None):
    """`KeccakRoundAir::eval` (round/mod.rs:206-311) and its `LookupAir::eval` (:396-560), both lanes."""
    from .chiplets_air import When
    b = dag.AirBuilder(KR_MAIN_COLS, aux_width=KR_AUX_COLS, num_randomness=NUM_RANDOMNESS, num_aux_values=NUM_SIGMA_VALUES,
                       num_public=NUM_PUBLIC_VALUES, periodic=keccak_round_program())
    w = When(b)
    per = [b.periodic_value(i) for i in range(10)]
    p_last, is_xor, is_andnot, is_rol, k = per[PCOL_P_LAST], per[PCOL_IS_XOR], per[PCOL_IS_ANDNOT], per[PCOL_IS_ROL], per[PCOL_K]
    two_32 = b.const(1 << 32)
    for lane in range(KR_NUM_LANES):
        base = lane * KR_LANE_WIDTH
        ip, next_ip = b.main(base + KR_COL_IP), b.main(base + KR_COL_IP, 1)
        act, next_act = b.main(base + KR_COL_ACT), b.main(base + KR_COL_ACT, 1)
        if lane == 0:
            w.when_first_row().assert_eq(ip, b.const(KR_IP_BOUNDARY))
        w.when_transition().assert_zero(next_ip - ip - 1)
        w.assert_bool(act)
        w.assert_zero((1 - p_last) * (next_act - act))
        no_logic = 1 - (is_xor + is_andnot)
        for i in range(8):
            w.assert_zero(no_logic * (b.main(base + KR_R + i) - b.main(base + KR_A + i)))
        r_bytes = [b.main(base + KR_R + i) for i in range(8)]
        rot = [b.main(base + KR_ROT + i) for i in range(8)]
        r_lo, r_hi = _pack_le(r_bytes[:4], 256), _pack_le(r_bytes[4:], 256)
        rol_gate = act * is_rol
        w.assert_zero(rol_gate * ((r_lo + two_32) * k - _pack_le(rot[:4], 1 << 16)))
        w.assert_zero(rol_gate * ((r_hi + two_32) * k - _pack_le(rot[4:], 1 << 16)))
    lk = dag.LogUp(b, MAX_MESSAGE_WIDTH, NUM_BUS_IDS, closing="sigma_last_row")

    def side(bb):
        p = [bb.periodic_value(i) for i in range(10)]
        return dict(bb=bb, p=p, one=bb.const(1), zero=bb.const(0))
    sc, sp = side(lk.b), side(lk.lb)

    def both(f):
        return f(sc), f(sp)

    def msg(f):
        def m(ch):
            bus, fields = f(sc if ch is lk.ch_c else sp)
            return ch.encode(bus, fields)
        return m

    def frac_col(*fracs):  # logup/mod.rs frac_col!: one group, one batch with flag ONE, its fractions
        with lk.column() as col:
            with col.group() as g:
                with g.batch(both(lambda s: s["one"])) as bt:
                    for mult, message in fracs:
                        bt.insert(mult, message)
    for lane in range(KR_NUM_LANES):
        base = lane * KR_LANE_WIDTH

        def cells(s, off, n=8):
            return [s["bb"].main(base + off + i) for i in range(n)]

        def gates(s):
            p = s["p"]
            act = s["bb"].main(base + KR_COL_ACT)
            return dict(is_active=act * (p[PCOL_IS_XOR] + p[PCOL_IS_ANDNOT] + p[PCOL_IS_ROL] - p[PCOL_IS_XORROL]),
                        reads_b=act * (p[PCOL_IS_XOR] + p[PCOL_IS_ANDNOT]), rol_act=act * p[PCOL_IS_ROL], dst=act * p[PCOL_DST_MULT],
                        logic_active=p[PCOL_IS_XOR] + p[PCOL_IS_ANDNOT], bpl_op=s["one"] - p[PCOL_IS_ANDNOT])

        def provide_c(s):  # `memory_provide_c` / `rotated_halves` (mod.rs:322-363)
            p = s["p"]
            r, limb = cells(s, KR_R), cells(s, KR_ROT)
            r_lo, r_hi = _pack_le(r[:4], 256), _pack_le(r[4:], 256)
            two_16 = s["bb"].const(1 << 16)
            c0, c1, c2, c3 = limb[0] + limb[6], limb[1] + limb[7], limb[2] + limb[4], limb[3] + limb[5]
            lo = c0 + c1 * two_16 - p[PCOL_K]
            hi = c2 + c3 * two_16 - p[PCOL_K]
            lo_f = lo + p[PCOL_SWAP] * (hi - lo)
            hi_f = hi + p[PCOL_SWAP] * (lo - hi)
            return r_lo + p[PCOL_IS_ROL] * (lo_f - r_lo), r_hi + p[PCOL_IS_ROL] * (hi_f - r_hi)

        def ip_of(s):
            return s["bb"].main(base + KR_COL_IP)
        # band col 0: the Memory64 dst provide
        frac_col((both(lambda s: s["zero"] - gates(s)["dst"]), msg(lambda s: (BUS_MEMORY64, [ip_of(s), *provide_c(s)]))))
        # band col 1: the src_a and src_b requires
        frac_col((both(lambda s: gates(s)["is_active"]),
                  msg(lambda s: (BUS_MEMORY64, [ip_of(s) - s["p"][PCOL_BACK_A], _pack_le(cells(s, KR_A)[:4], 256), _pack_le(cells(s, KR_A)[4:], 256)]))),
                 (both(lambda s: gates(s)["reads_b"]),
                  msg(lambda s: (BUS_MEMORY64, [ip_of(s) - s["p"][PCOL_BACK_B], _pack_le(cells(s, KR_B)[:4], 256), _pack_le(cells(s, KR_B)[4:], 256)]))))
        # band cols 2-5: eight byte requests, two per column
        for pair in range(4):
            def byte_req(i):
                return (both(lambda s: gates(s)["is_active"]),
                        msg(lambda s: (BUS_BYTE_PAIR_LUT, [gates(s)["bpl_op"], cells(s, KR_A)[i], gates(s)["logic_active"] * cells(s, KR_B)[i], cells(s, KR_R)[i]])))
            frac_col(byte_req(2 * pair), byte_req(2 * pair + 1))
        # band cols 6-9: eight Range16 requests on the rotation limbs
        for pair in range(4):
            def limb_req(i):
                return (both(lambda s: gates(s)["rol_act"]), msg(lambda s: (BUS_RANGE16, [cells(s, KR_ROT)[i]])))
            frac_col(limb_req(2 * pair), limb_req(2 * pair + 1))
    lookup = lk.finish("keccak_round")
    return dag.Air(b, _host_aux(lookup, host_aux), "keccak_round"), lookup


# ---- KeccakSponge: pad10*1, absorb, squeeze around the round chiplet's permutations (hash/keccak/sponge/{mod,program,message,trace}.rs) ---
# One row per state lane, a period of 32 rows per Keccak-f permutation (sponge row r = 32 n + idx  <->  the round chiplet's address
# 3200 n + idx: every per-row address is linear in `sponge_seq_id` and the periodic `p_idx`).  Slots 0..16 XOR the rate lanes in
# (verbatim, or through the pad row's ANDNOT / XOR 0x01 / XOR chain, or not at all past the pad), 17..24 pass the capacity through, 25
# mixes the trailing 0x80 into lane 16 on last blocks, 26..28 mop up the chunk lanes a last block leaves over, 29..31 idle.  The rows
# provide the permutation's input lanes and round constants on Memory64, consume the previous permutation's outputs (inside an
# invocation) or the squeezed lanes 4..24 (last block), consume the input from the chunk chiplet's tape, verify every XOR / ANDNOT byte
# by byte against the byte-pair table, and consume one `KeccakSponge` request per invocation.  67 main columns (5 structural, 10 of the
# padding state machine, 12 lane halves, 40 byte shadows), 24 flattened LogUp columns, 11 periodic columns, log_quotient_degree 2.
SP_COLS, SP_AUX_COLS, SPONGE_PERIOD, SP_NUM_PERIODIC = 67, 24, 32, 11                                        # sponge/mod.rs:165, :190; program.rs:3-4
SPC_SEQ_ID, SPC_ACT, SPC_BYTES_LEFT, SPC_IS_FIRST_BLOCK, SPC_CHUNK_PTR, SPC_IS_ZERO, SPC_IS_CHUNK_AVAIL, SPC_B = 0, 1, 2, 3, 4, 5, 6, 7
SPC_CHUNK, SPC_STATE_PREV, SPC_STATE_NEW, SPC_STATE_OUT, SPC_CLEARED, SPC_PADDED = 15, 17, 19, 21, 23, 25      # `_LO`; `_HI` = + 1
SPC_CHUNK_BYTES, SPC_STATE_PREV_BYTES, SPC_STATE_NEW_BYTES, SPC_CLEARED_BYTES, SPC_PADDED_BYTES = 27, 35, 43, 51, 59
(SPP_IDX, SPP_FIRST, SPP_LAST, SPP_RATE_BLOCK, SPP_CAPACITY, SPP_RC_ACTIVE, SPP_SQUEEZE_ACTIVE, SPP_PAD_0X80, SPP_RC_LO, SPP_RC_HI,
 SPP_EXTRA) = range(11)                                                                                        # program.rs:5-15
SP_RATE_LANES, SP_RATE_BYTES, SP_LANE16_SLOT, SP_EXTRA_BEGIN, SP_NOP_BEGIN = 17, 136, 25, 26, 29                 # program.rs:16-24
SP_PAD_CONST = 0x8000000000000000                                                                               # trace.rs:62


def sponge_program():
    """`sponge_program` (sponge/program.rs:52-74) -> 11 columns of 32."""
    cols = [[0] * SPONGE_PERIOD for _ in range(SP_NUM_PERIODIC)]
    for slot in range(SPONGE_PERIOD):
        cols[SPP_IDX][slot] = slot
        cols[SPP_FIRST][slot] = int(slot == 0)
        cols[SPP_LAST][slot] = int(slot == SPONGE_PERIOD - 1)
        cols[SPP_RATE_BLOCK][slot] = int(slot < SP_RATE_LANES)
        cols[SPP_CAPACITY][slot] = int(SP_RATE_LANES <= slot < SP_LANE16_SLOT)
        cols[SPP_RC_ACTIVE][slot] = int(slot < 24)
        cols[SPP_SQUEEZE_ACTIVE][slot] = int(4 <= slot < SP_LANE16_SLOT)
        cols[SPP_PAD_0X80][slot] = int(slot == SP_LANE16_SLOT)
        cols[SPP_EXTRA][slot] = int(SP_EXTRA_BEGIN <= slot < SP_NOP_BEGIN)
        if slot < 24:
            cols[SPP_RC_LO][slot], cols[SPP_RC_HI][slot] = KECCAK_RC[slot] & 0xffffffff, KECCAK_RC[slot] >> 32
    return cols


def _sp_andnot_mask(j):     # trace.rs `andnot_mask`: 0xff..ff << 8 j (mod.rs ANDNOT_MASK_{LO,HI})
    return (0xffffffffffffffff << (8 * j)) & 0xffffffffffffffff


def _sp_padding_mask(j):    # trace.rs `padding_mask`: 0x01 << 8 j (mod.rs PADDING_MASK_{LO,HI})
    return 1 << (8 * j)


def keccak_sponge_air(host_aux=None):
    """`KeccakSpongeAir::eval` (hash/keccak/sponge/mod.rs:356-598) and its `LookupAir::eval` (:631-1046)."""
    b = dag.AirBuilder(SP_COLS, aux_width=SP_AUX_COLS, num_randomness=NUM_RANDOMNESS, num_aux_values=NUM_SIGMA_VALUES,
                       num_public=NUM_PUBLIC_VALUES, periodic=sponge_program())
    loc, nxt = [b.main(c) for c in range(SP_COLS)], [b.main(c, 1) for c in range(SP_COLS)]
    one = b.const(1)
    per = [b.periodic_value(i) for i in range(SP_NUM_PERIODIC)]
    p_first, p_last, p_rate_block, p_capacity, p_extra = per[SPP_FIRST], per[SPP_LAST], per[SPP_RATE_BLOCK], per[SPP_CAPACITY], per[SPP_EXTRA]
    p_state_lane = p_rate_block + p_capacity
    act, act_next = loc[SPC_ACT], nxt[SPC_ACT]
    seq, seq_next = loc[SPC_SEQ_ID], nxt[SPC_SEQ_ID]
    bytes_left, bytes_left_next = loc[SPC_BYTES_LEFT], nxt[SPC_BYTES_LEFT]
    chunk_ptr, chunk_ptr_next = loc[SPC_CHUNK_PTR], nxt[SPC_CHUNK_PTR]
    ifb, ifb_next = loc[SPC_IS_FIRST_BLOCK], nxt[SPC_IS_FIRST_BLOCK]
    is_zero, is_zero_next = loc[SPC_IS_ZERO], nxt[SPC_IS_ZERO]
    ica, ica_next = loc[SPC_IS_CHUNK_AVAIL], nxt[SPC_IS_CHUNK_AVAIL]
    sp_lo, sp_hi, sn_lo, sn_hi = loc[SPC_STATE_PREV], loc[SPC_STATE_PREV + 1], loc[SPC_STATE_NEW], loc[SPC_STATE_NEW + 1]
    b_sum, b_weighted = b.const(0), b.const(0)
    for j in range(8):
        b_sum = b_sum + loc[SPC_B + j]
        b_weighted = b_weighted + b.const(j) * loc[SPC_B + j]

    def bool_check(x):
        b.assert_zero((one - x) * x)
    tr, first = b.is_transition(), b.is_first_row()
    b.assert_zero(first * seq)
    bool_check(act)
    b.assert_zero(tr * ((one - act) * act_next))
    b.assert_zero(tr * ((act - act_next) * (one - p_last * b_sum)))
    b.assert_zero(tr * (seq_next - seq - one))
    bool_check(ifb)
    b.assert_zero((one - p_last) * (ifb_next - ifb))
    b.assert_zero(act * p_rate_block * (bytes_left_next - bytes_left + b.const(8)))
    enters = p_last * ifb_next
    b.assert_zero(act * (one - enters) * (one - p_rate_block) * (bytes_left_next - bytes_left))
    b.assert_zero(tr * ((one - enters) * (chunk_ptr_next - chunk_ptr - (p_rate_block + p_extra * b_sum) * ica)))
    b.assert_zero((one - ica) * loc[SPC_CHUNK])
    b.assert_zero((one - ica) * loc[SPC_CHUNK + 1])
    bool_check(is_zero)
    bool_check(ica)
    for j in range(8):
        bool_check(loc[SPC_B + j])
    b.assert_zero((one - p_last) * is_zero * (one - is_zero_next))
    b.assert_zero((one - p_last) * (one - ica) * ica_next)
    b.assert_zero(p_first * is_zero)
    for j in range(8):
        b.assert_zero((one - p_last) * (nxt[SPC_B + j] - loc[SPC_B + j]))
    b.assert_zero((one - p_rate_block) * (b_sum - is_zero))
    b.assert_zero(act * p_last * ifb_next * (one - is_zero))
    is_pad = is_zero_next - is_zero
    b.assert_zero(p_rate_block * is_pad * (b_weighted - bytes_left))
    b.assert_zero(p_state_lane * ifb * sp_lo)
    b.assert_zero(p_state_lane * ifb * sp_hi)
    b.assert_zero(p_rate_block * is_zero * (sn_lo - sp_lo))
    b.assert_zero(p_rate_block * is_zero * (sn_hi - sp_hi))
    b.assert_zero(p_capacity * (sn_lo - sp_lo))
    b.assert_zero(p_capacity * (sn_hi - sp_hi))
    for bytes_at, half_at in ((SPC_CHUNK_BYTES, SPC_CHUNK), (SPC_STATE_PREV_BYTES, SPC_STATE_PREV), (SPC_STATE_NEW_BYTES, SPC_STATE_NEW),
                              (SPC_CLEARED_BYTES, SPC_CLEARED), (SPC_PADDED_BYTES, SPC_PADDED)):      # byte-shadow linking, utils.rs `halves_le`
        b.assert_zero(_pack_le(loc[bytes_at:bytes_at + 4], 256) - loc[half_at])
        b.assert_zero(_pack_le(loc[bytes_at + 4:bytes_at + 8], 256) - loc[half_at + 1])

    lk = dag.LogUp(b, MAX_MESSAGE_WIDTH, NUM_BUS_IDS, closing="sigma_last_row")

    class Side:
        def __init__(self, bb):
            self.bb = bb
            c = bb.const
            row, nrow = [bb.main(i) for i in range(SP_COLS)], [bb.main(i, 1) for i in range(SP_COLS)]
            pv = [bb.periodic_value(i) for i in range(SP_NUM_PERIODIC)]
            self.row = row
            p_state_lane_ = pv[SPP_RATE_BLOCK] + pv[SPP_CAPACITY]
            act_ = row[SPC_ACT]
            b_sum_ = c(0)
            self.andnot_mask_bytes, self.padding_mask_bytes = [c(0)] * 8, [c(0)] * 8
            for j in range(8):
                b_j = row[SPC_B + j]
                b_sum_ = b_sum_ + b_j
                for i in range(8):
                    self.andnot_mask_bytes[i] = self.andnot_mask_bytes[i] + c((_sp_andnot_mask(j) >> (8 * i)) & 0xff) * b_j
                    self.padding_mask_bytes[i] = self.padding_mask_bytes[i] + c((_sp_padding_mask(j) >> (8 * i)) & 0xff) * b_j
            is_intra = c(1) - row[SPC_IS_FIRST_BLOCK]
            is_first_row_of_invocation = pv[SPP_FIRST] * row[SPC_IS_FIRST_BLOCK]
            is_pad_ = nrow[SPC_IS_ZERO] - row[SPC_IS_ZERO]
            is_verbatim = c(1) - nrow[SPC_IS_ZERO]
            hundred_seq = c(100) * row[SPC_SEQ_ID]
            ninety_nine_idx = c(99) * pv[SPP_IDX]
            self.addr_prev = hundred_seq - ninety_nine_idx - c(128)
            self.addr_new = hundred_seq - ninety_nine_idx
            self.addr_rc = hundred_seq + c(28) * pv[SPP_IDX] + c(25)
            self.addr_squeeze = hundred_seq - ninety_nine_idx + c(3072)
            self.addr_lane16 = hundred_seq - c(2484)
            self.addr_chunk = c(CHUNK_ADDR_BASE) + row[SPC_CHUNK_PTR]
            mult_prev_perm = c(2) * act_ * is_intra
            mult_new_state = c(0) - c(2) * act_
            mult_rc = c(0) - c(1) * act_ * pv[SPP_RC_ACTIVE]
            mult_squeeze = c(2) * act_ * pv[SPP_SQUEEZE_ACTIVE] * b_sum_
            mult_lane16_consume = c(2) * act_ * b_sum_
            mult_lane16_provide = c(0) - c(2) * act_ * b_sum_
            self.m = dict(new_state=p_state_lane_ * mult_new_state, prev_perm=p_state_lane_ * mult_prev_perm, rc=p_state_lane_ * mult_rc,
                          lane16_consume=pv[SPP_PAD_0X80] * mult_lane16_consume, lane16_provide=pv[SPP_PAD_0X80] * mult_lane16_provide,
                          squeeze=p_state_lane_ * mult_squeeze, pad=pv[SPP_RATE_BLOCK] * is_pad_ * act_,
                          verbatim=pv[SPP_RATE_BLOCK] * is_verbatim * act_, lane16=pv[SPP_PAD_0X80] * b_sum_ * act_,
                          ks_request=act_ * is_first_row_of_invocation,
                          chunk_consume=act_ * (pv[SPP_RATE_BLOCK] + pv[SPP_EXTRA] * b_sum_) * row[SPC_IS_CHUNK_AVAIL])
            self.rc_lo, self.rc_hi = pv[SPP_RC_LO], pv[SPP_RC_HI]

    sides = {id(lk.ch_c): Side(lk.b), id(lk.ch_p): Side(lk.lb)}

    def mult(name):
        return sides[id(lk.ch_c)].m[name], sides[id(lk.ch_p)].m[name]

    def mem64(addr, half_at=None, rc=False):
        def msg(ch):
            s_ = sides[id(ch)]
            lo, hi = (s_.rc_lo, s_.rc_hi) if rc else (s_.row[half_at], s_.row[half_at + 1])
            return ch.encode(BUS_MEMORY64, [getattr(s_, addr), lo, hi])
        return msg

    def bpl(op, a, bsrc, csrc, i):
        """BytePairLutMsg { op, a, b, c } on byte i; a source is a column base, ("andnot" | "padding") for the mask bytes, or an int table."""
        def pick(s_, src):
            if src == "andnot":
                return s_.andnot_mask_bytes[i]
            if src == "padding":
                return s_.padding_mask_bytes[i]
            if isinstance(src, tuple):
                return s_.bb.const(src[i])
            return s_.row[src + i]

        def msg(ch):
            s_ = sides[id(ch)]
            return ch.encode(BUS_BYTE_PAIR_LUT, [s_.bb.const(op), pick(s_, a), pick(s_, bsrc), pick(s_, csrc)])
        return msg

    def ks_request(ch):
        s_ = sides[id(ch)]
        return ch.encode(BUS_KECCAK_SPONGE, [s_.row[SPC_SEQ_ID], s_.row[SPC_CHUNK_PTR], s_.row[SPC_BYTES_LEFT]])

    pad_const_bytes = tuple((SP_PAD_CONST >> (8 * i)) & 0xff for i in range(8))
    columns = [[(mult("new_state"), mem64("addr_new", SPC_STATE_NEW)), (mult("prev_perm"), mem64("addr_prev", SPC_STATE_PREV))],
               [(mult("rc"), mem64("addr_rc", rc=True)), (mult("lane16_consume"), mem64("addr_lane16", SPC_STATE_PREV)),
                (mult("lane16_provide"), mem64("addr_lane16", SPC_STATE_NEW))],
               [(mult("squeeze"), mem64("addr_squeeze", SPC_STATE_OUT))]]
    for m_name, op, a, bsrc, csrc in (("pad", OP_ANDNOT, "andnot", SPC_CHUNK_BYTES, SPC_CLEARED_BYTES),
                                      ("pad", OP_XOR, SPC_CLEARED_BYTES, "padding", SPC_PADDED_BYTES),
                                      ("pad", OP_XOR, SPC_STATE_PREV_BYTES, SPC_PADDED_BYTES, SPC_STATE_NEW_BYTES),
                                      ("verbatim", OP_XOR, SPC_STATE_PREV_BYTES, SPC_CHUNK_BYTES, SPC_STATE_NEW_BYTES),
                                      ("lane16", OP_XOR, SPC_STATE_PREV_BYTES, pad_const_bytes, SPC_STATE_NEW_BYTES)):
        for pair in range(4):
            columns.append([(mult(m_name), bpl(op, a, bsrc, csrc, 2 * pair)), (mult(m_name), bpl(op, a, bsrc, csrc, 2 * pair + 1))])
    columns.append([(mult("ks_request"), ks_request), (mult("chunk_consume"), mem64("addr_chunk", SPC_CHUNK))])
    assert len(columns) == SP_AUX_COLS
    for fractions in columns:
        with lk.column() as col:
            with col.group() as g:
                with g.batch((lk.b.const(1), lk.lb.const(1))) as bt:
                    for m_, msg in fractions:
                        bt.insert(m_, msg)
    lookup = lk.finish("keccak_sponge")
    return dag.Air(b, _host_aux(lookup, host_aux), "keccak_sponge"), lookup


# ---- KeccakNode: one Keccak invocation = one transcript-DAG node (hash/keccak/node/{mod,trace}.rs) ------------------------------------------
# One row per DISTINCT hashed input.  The row issues the sponge's `KeccakSponge` request, consumes the chunk chain's `ChunkChain` tuple,
# reads the four digest lanes D off the round chiplet's outputs (twice each, as they are provided), drives two Poseidon2 permutations --
# H_digest_chunks = hash of D as a one-chunk payload under `Tag::CHUNKS`, H_keccak = hash of [H_input_chunks | H_digest_chunks] under the
# Keccak-256 assertion tag [precompile id, 0, len_bytes, 0] -- reads H_input_chunks at the tail of the chunk chain, and provides
# `Binding(H_keccak, True, 0, 0)` once per reader.  30 main columns, nine flattened LogUp columns, no periodic columns, lqd 1.
KN_COLS, KN_AUX_COLS = 30, 9                                                                                  # node/mod.rs:122-153
(KNC_ACT, KNC_SPONGE_HEAD, KNC_N_PERMS, KNC_CHUNK_HEAD, KNC_N_CHUNKS, KNC_PERM_CHUNKS, KNC_LEN, KNC_PERM_DIGEST_CHUNKS, KNC_PERM_KECCAK,
 KNC_D) = range(10)
KNC_H_INPUT_CHUNKS, KNC_H_DIGEST_CHUNKS, KNC_H_KECCAK, KNC_OUT_MULT = 17, 21, 25, 29
# `Keccak256Precompile::id()` = `precompile_id("keccak256")` (core/src/deferred/precompile.rs:68-78): the first eight bytes, little-endian,
# of BLAKE3("miden-deferred-precompile/v1:9:keccak256"); checked against the library's BLAKE3 in tests/test_precompile_node.py
KECCAK256_PRECOMPILE_ID = 1416710563871706399
KECCAK256_ASSERT_TAG_ID = 0                                                                                     # precompiles/src/hash/mod.rs:39, :66
VALUE_TAG_TRUE = 0                                                                                              # transcript/binding.rs:38-46


def _node_local(b, off=0):
    """The local constraints of `KeccakNodeAir::eval` (hash/keccak/node/mod.rs:196-262) over the main columns [off, off + 30)."""
    loc, nxt = [b.main(off + c) for c in range(KN_COLS)], [b.main(off + c, 1) for c in range(KN_COLS)]
    one = b.const(1)
    act, act_next = loc[KNC_ACT], nxt[KNC_ACT]
    b.assert_zero(b.is_first_row() * loc[KNC_SPONGE_HEAD])
    b.assert_zero(b.is_first_row() * loc[KNC_CHUNK_HEAD])
    b.assert_zero((one - act) * act)
    b.assert_zero(b.is_transition() * ((one - act) * act_next))
    b.assert_zero((one - act) * loc[KNC_OUT_MULT])
    b.assert_zero(b.is_transition() * (act_next * (nxt[KNC_SPONGE_HEAD] - loc[KNC_SPONGE_HEAD] - b.const(32) * loc[KNC_N_PERMS])))
    b.assert_zero(b.is_transition() * (act_next * (nxt[KNC_CHUNK_HEAD] - loc[KNC_CHUNK_HEAD] - loc[KNC_N_CHUNKS])))


def _node_columns(lk, off=0):
    """The nine flattened LogUp columns of `KeccakNodeAir` (hash/keccak/node/mod.rs:287-559) -> [[(multiplicity pair, message)]]."""
    def side(ch):
        bb = lk.b if ch is lk.ch_c else lk.lb
        return bb, [bb.main(off + c) for c in range(KN_COLS)]

    def ks_request(ch):
        bb, r = side(ch)
        return ch.encode(BUS_KECCAK_SPONGE, [r[KNC_SPONGE_HEAD], bb.const(4) * r[KNC_CHUNK_HEAD], r[KNC_LEN]])

    def binding(ch):       # BindingMsg::truth(h_keccak) (transcript/binding.rs:74-81, :109-121)
        bb, r = side(ch)
        return ch.encode(BUS_BINDING, r[KNC_H_KECCAK:KNC_H_KECCAK + 4] + [bb.const(VALUE_TAG_TRUE), bb.const(0), bb.const(0)])

    def chunk_chain(ch):
        _, r = side(ch)
        return ch.encode(BUS_CHUNK_CHAIN, [r[KNC_CHUNK_HEAD], r[KNC_PERM_CHUNKS]])

    def p2_out(perm, at):
        def msg(ch):
            bb, r = side(ch)
            perm_seq_id = r[KNC_PERM_CHUNKS] + r[KNC_N_CHUNKS] - bb.const(1) if perm is None else r[perm]
            return ch.encode(BUS_POSEIDON2_OUT, [perm_seq_id] + r[at:at + 4])
        return msg

    def d_lane(j):
        def msg(ch):
            bb, r = side(ch)
            base = bb.const(100) * r[KNC_SPONGE_HEAD] + bb.const(3200) * r[KNC_N_PERMS] - bb.const(128)
            return ch.encode(BUS_MEMORY64, [base + bb.const(j), r[KNC_D + 2 * j], r[KNC_D + 2 * j + 1]])
        return msg

    def p2_in(perm, tag, src):
        def msg(ch):
            bb, r = side(ch)
            if src == "cap_chunks":
                c = [bb.const(x) for x in TAG_CHUNKS_WORD]
            elif src == "cap_keccak":
                c = [bb.const(KECCAK256_PRECOMPILE_ID), bb.const(KECCAK256_ASSERT_TAG_ID), r[KNC_LEN], bb.const(0)]
            else:
                c = r[src:src + 4]
            return ch.encode(BUS_POSEIDON2_IN, [r[perm], bb.const(tag)] + c)
        return msg

    def mults(fn):
        return fn(lk.b), fn(lk.lb)
    neg_act = mults(lambda bb: bb.const(0) - bb.main(off + KNC_ACT))
    pos_act = mults(lambda bb: bb.main(off + KNC_ACT))
    pos_act_x2 = mults(lambda bb: bb.const(2) * bb.main(off + KNC_ACT))
    neg_out_mult = mults(lambda bb: bb.const(0) - bb.main(off + KNC_OUT_MULT))
    dc, kk = KNC_PERM_DIGEST_CHUNKS, KNC_PERM_KECCAK
    return [[(neg_act, ks_request)], [(neg_out_mult, binding), (pos_act, chunk_chain)], [(pos_act, p2_out(None, KNC_H_INPUT_CHUNKS))],
            [(pos_act_x2, d_lane(0)), (pos_act_x2, d_lane(1))], [(pos_act_x2, d_lane(2)), (pos_act_x2, d_lane(3))],
            [(pos_act, p2_in(dc, POSEIDON2_IN_TAG_RATE0, KNC_D)), (pos_act, p2_in(dc, POSEIDON2_IN_TAG_RATE1, KNC_D + 4))],
            [(pos_act, p2_in(dc, POSEIDON2_IN_TAG_CAP, "cap_chunks")), (pos_act, p2_out(dc, KNC_H_DIGEST_CHUNKS))],
            [(pos_act, p2_in(kk, POSEIDON2_IN_TAG_RATE0, KNC_H_INPUT_CHUNKS)), (pos_act, p2_in(kk, POSEIDON2_IN_TAG_RATE1, KNC_H_DIGEST_CHUNKS))],
            [(pos_act, p2_in(kk, POSEIDON2_IN_TAG_CAP, "cap_keccak")), (pos_act, p2_out(kk, KNC_H_KECCAK))]]


def keccak_node_air(host_aux=None):
    """`KeccakNodeAir::eval` (hash/keccak/node/mod.rs:196-262) and its `LookupAir::eval` (:287-559): col 0 the KeccakSponge request |
    col 1 Binding provide + ChunkChain consume | col 2 Poseidon2Out(H_input_chunks) | cols 3-4 the four digest lanes | cols 5-6 the
    digest-chunks permutation | cols 7-8 the Keccak-node permutation."""
    b = dag.AirBuilder(KN_COLS, aux_width=KN_AUX_COLS, num_randomness=NUM_RANDOMNESS, num_aux_values=NUM_SIGMA_VALUES,
                       num_public=NUM_PUBLIC_VALUES)
    _node_local(b)
    lk = dag.LogUp(b, MAX_MESSAGE_WIDTH, NUM_BUS_IDS, closing="sigma_last_row")
    columns = _node_columns(lk)
    assert len(columns) == KN_AUX_COLS
    _emit_frac_cols(lk, columns)
    lookup = lk.finish("keccak_node")
    return dag.Air(b, _host_aux(lookup, host_aux), "keccak_node"), lookup


# ---- ChunkNode: the chunk chiplet and the Keccak node chiplet on one row range (hash/chunk_node/{mod,trace}.rs) ---------------------------
# What `ChipletAir::all()` (session/prove.rs:111-126) actually runs: both period-1 AIRs side by side in disjoint column ranges -- main
# columns 0..12 = ChunkAir's layout, 12..42 = KeccakNodeAir's, LogUp columns 0..5 = the chunk's (column 0 its anchor), 5..14 = the
# node's (its anchor an ordinary column here); no mode selector, no cross-gating, one sigma; the height = the larger of the two.
CN_COLS, CN_AUX_COLS, CN_NODE_OFFSET = CHUNK_COLS + KN_COLS, CHUNK_AUX_COLS + KN_AUX_COLS, CHUNK_COLS


def chunk_node_air(host_aux=None):
    """`ChunkNodeAir::eval` (hash/chunk_node/mod.rs:106-190: the chunk's seven constraints, then the node's seven) and its `LookupAir::eval`
    (the chunk's five columns, then the node's nine: COLUMN_SHAPE [1, 2, 2, 2, 1, 1, 2, 1, 2, 2, 2, 2, 2, 2])."""
    b = dag.AirBuilder(CN_COLS, aux_width=CN_AUX_COLS, num_randomness=NUM_RANDOMNESS, num_aux_values=NUM_SIGMA_VALUES,
                       num_public=NUM_PUBLIC_VALUES)
    _chunk_local(b)
    _node_local(b, CN_NODE_OFFSET)
    lk = dag.LogUp(b, MAX_MESSAGE_WIDTH, NUM_BUS_IDS, closing="sigma_last_row")
    columns = _chunk_columns(lk) + _node_columns(lk, CN_NODE_OFFSET)
    assert [len(c) for c in columns] == [1, 2, 2, 2, 1, 1, 2, 1, 2, 2, 2, 2, 2, 2]
    _emit_frac_cols(lk, columns)
    lookup = lk.finish("chunk_node")
    return dag.Air(b, _host_aux(lookup, host_aux), "chunk_node"), lookup


# ---- UintAdd: a + b = c (mod p) over stored 256-bit values (uint/add/{mod,trace}.rs) -------------------------------------------------------
# A relation AIR over the uint store: a, b, c and the modulus (stored as bound = p - 1) are pulled in over `UintVal`, the chiplet ties
# their pointers to the modular-sum identity and provides `UintAdd(bound_ptr, a_ptr, b_ptr, c_ptr, nz)`.  The identity is checked by a
# "vertical Schwartz-Zippel": with the eight 32-bit limbs of each value as coefficients,
#     a(beta) + b(beta) - c(beta) - k (bound(beta) + 1) + (beta - 2^32) Gamma(beta) = 0,   Gamma = seven ternary carries,
# at the LogUp challenge beta -- ONE extension-field constraint on the two-row window of a block (open row a || b, closing row c || p),
# no accumulator column.  Two zero-sentinel modes (is_c_zero: a + b = 0, negation; is_b_zero: a = c, the equality certificate) and a
# nonzero certificate for b (nz: w * sum of b's limbs = 1).  30 main columns, three LogUp columns, one periodic selector of period 2, lqd 1.
UA_COLS, UA_AUX_COLS, UA_NUM_LIMBS, UA_PERIOD = 30, 3, 8, 2                                                    # uint/add/mod.rs:146-171
UA_CELL_HI, UA_CELL_FLAG, UA_CELL_W, UA_CELL_WS, UA_CELL_B_ON = 8, 20, 21, 22, 23                               # open row: is_b_zero | w | wS | b_on
UA_CELL_K, UA_CELL_C_ON, UA_CELL_MULT, UA_CELL_IS_C_ZERO = 20, 21, 22, 23                                       # closing row: k | c_on | mult | is_c_zero
UA_COL_A_PTR, UA_COL_B_PTR, UA_COL_C_PTR, UA_COL_BOUND_PTR, UA_COL_ACT, UA_COL_NZ = 24, 25, 26, 27, 28, 29
UA_GAMMA_SLOTS = ((0, 16), (0, 17), (0, 18), (0, 19), (1, 16), (1, 17), (1, 18))                               # (block row, cell) of gamma_0..6


def uint_add_air(host_aux=None):
    """`UintAddAir::eval` (uint/add/mod.rs:262-474) and its `LookupAir::eval` (:534-633): col 0 the `a` consume | col 1 the gated `b` and
    `c` consumes | col 2 the modulus consume + the UintAdd provide."""
    b = dag.AirBuilder(UA_COLS, aux_width=UA_AUX_COLS, num_randomness=NUM_RANDOMNESS, num_aux_values=NUM_SIGMA_VALUES,
                       num_public=NUM_PUBLIC_VALUES, periodic=[[1, 0]])
    loc, nxt = [b.main(c) for c in range(UA_COLS)], [b.main(c, 1) for c in range(UA_COLS)]
    one = b.const(1)
    ab_sel = b.periodic_value(0)
    cp_sel = one - ab_sel
    beta = b.randomness(1)
    bp = [b.const(1)]
    for _ in range(1, 8):
        bp.append(bp[-1] * beta)
    t32 = b.const(1 << 32)

    def at_beta(cells):
        acc = b.const(0)
        for j in range(UA_NUM_LIMBS):
            acc = acc + bp[j] * cells[j]
        return acc
    a_beta, b_beta = at_beta(loc[0:8]), at_beta(loc[UA_CELL_HI:UA_CELL_HI + 8])
    c_beta, p_beta = at_beta(nxt[0:8]), at_beta(nxt[UA_CELL_HI:UA_CELL_HI + 8])
    is_b_zero, is_c_zero_next, k_next = loc[UA_CELL_FLAG], nxt[UA_CELL_IS_C_ZERO], nxt[UA_CELL_K]
    carry = b.const(0)
    for j, (row, cell) in enumerate(UA_GAMMA_SLOTS):
        w = bp[j + 1] - bp[j] * t32
        carry = carry + w * (loc[cell] if row == 0 else nxt[cell])
    identity = a_beta + b_beta * (one - is_b_zero) - c_beta * (one - is_c_zero_next) - (p_beta + bp[0]) * k_next + carry
    b.assert_zero_ext(identity * ab_sel)
    for cell in range(16, 20):                                          # ternary carries, ungated
        g = loc[cell]
        b.assert_zero(g * (one - g) * (one + g))
    for col in (UA_CELL_FLAG, UA_CELL_B_ON):                            # a boolean on both rows of the block
        b.assert_zero(loc[col] * (one - loc[col]))
    act, nz = loc[UA_COL_ACT], loc[UA_COL_NZ]
    b.assert_zero(act * (one - act))
    b.assert_zero(nz * (one - nz))
    b.assert_zero(cp_sel * (one - act) * loc[UA_CELL_MULT])
    is_c_zero = loc[UA_CELL_IS_C_ZERO]
    b.assert_zero(cp_sel * is_c_zero * loc[UA_COL_C_PTR])
    b.assert_zero(ab_sel * is_b_zero * loc[UA_COL_B_PTR])
    b.assert_zero(ab_sel * (loc[UA_CELL_B_ON] - act * (one - is_b_zero)))
    b.assert_zero(cp_sel * (loc[UA_CELL_C_ON] - act * (one - is_c_zero)))
    s_sum = b.const(0)
    for j in range(UA_NUM_LIMBS):
        s_sum = s_sum + loc[UA_CELL_HI + j]
    w_, ws = loc[UA_CELL_W], loc[UA_CELL_WS]
    b.assert_zero(ab_sel * (ws - w_ * s_sum))
    b.assert_zero(ab_sel * nz * (ws - one))
    for col in (UA_COL_A_PTR, UA_COL_B_PTR, UA_COL_C_PTR, UA_COL_BOUND_PTR, UA_COL_ACT, UA_COL_NZ):
        b.assert_zero(ab_sel * (nxt[col] - loc[col]))

    lk = dag.LogUp(b, MAX_MESSAGE_WIDTH, NUM_BUS_IDS, closing="sigma_last_row")

    def side(ch):
        bb = lk.b if ch is lk.ch_c else lk.lb
        return bb, [bb.main(c) for c in range(UA_COLS)]

    def uint_val(ptr_col, lo):           # UintValMsg { ptr, bound_ptr, limbs } (uint/mod.rs:116-134)
        def msg(ch):
            _, r = side(ch)
            return ch.encode(BUS_UINT_VAL, [r[ptr_col], r[UA_COL_BOUND_PTR]] + r[lo:lo + 8])
        return msg

    def uint_add(ch):                    # UintAddMsg (uint/add/mod.rs:116-141)
        _, r = side(ch)
        return ch.encode(BUS_UINT_ADD, [r[UA_COL_BOUND_PTR], r[UA_COL_A_PTR], r[UA_COL_B_PTR], r[UA_COL_C_PTR], r[UA_COL_NZ]])

    def mults(fn):
        return fn(lk.b), fn(lk.lb)

    def sel(bb, closing):
        return bb.const(1) - bb.periodic_value(0) if closing else bb.periodic_value(0)
    m_a = mults(lambda bb: sel(bb, False) * bb.main(UA_COL_ACT))
    m_b = mults(lambda bb: sel(bb, False) * bb.main(UA_CELL_B_ON))
    m_c = mults(lambda bb: sel(bb, True) * bb.main(UA_CELL_C_ON))
    m_p = mults(lambda bb: sel(bb, True) * bb.main(UA_COL_ACT))
    m_provide = mults(lambda bb: (bb.const(0) - bb.main(UA_CELL_MULT)) * sel(bb, True))
    _emit_frac_cols(lk, [[(m_a, uint_val(UA_COL_A_PTR, 0))], [(m_b, uint_val(UA_COL_B_PTR, UA_CELL_HI)), (m_c, uint_val(UA_COL_C_PTR, 0))],
                         [(m_p, uint_val(UA_COL_BOUND_PTR, UA_CELL_HI)), (m_provide, uint_add)]])
    lookup = lk.finish("uint_add")
    return dag.Air(b, _host_aux(lookup, host_aux), "uint_add"), lookup


# ---- EcPointStore: the points of the curves, their bindings and the curve-membership trio (ec/{mod,trace,require}.rs) ----------------
# One row = one point: its pointer (consecutive from 1 while `act`), its group's five-tuple (pulled from EcGroupsAir over `EcGroup`), the
# pointers of x and y in the uint store, and either the membership certificate u = x^2 + a, w = x u + b, y^2 = w as three consumed
# `UintMul` relations, or the flag of the point at infinity (no coordinates, no trio), or a closure certificate consumed from EcGroupAdd
# (`is_cert`: a sum of two points of the curve is on the curve).  Provides `EcPoint(ptr, group, x_ptr, y_ptr, is_pai)` to its readers.
# 14 main columns, five LogUp columns, lqd 1.
BUS_UINT_MUL, BUS_EC_POINT, BUS_EC_ON_CURVE_CERT = 12, 15, 17                                                   # relations.rs:52-80
EP_COLS, EP_AUX_COLS = 14, 5                                                                                    # ec/mod.rs:153-197
(EP_COL_PTR, EP_COL_GROUP_PTR, EP_COL_A_PTR, EP_COL_B_PTR, EP_COL_BOUND_PTR, EP_COL_SBOUND_PTR, EP_COL_X_PTR, EP_COL_Y_PTR, EP_COL_U_PTR,
 EP_COL_W_PTR, EP_COL_IS_PAI, EP_COL_ECPOINT_MULT, EP_COL_ACT, EP_COL_IS_CERT) = range(14)


def ec_point_store_air(host_aux=None):
    """`EcPointStoreAir::eval` (ec/mod.rs:238-290) and its `LookupAir::eval` (:316-463): col 0 the EcPoint provide | col 1 the EcGroup
    consume + the closure-certificate consume | cols 2-4 the membership trio u, w, y (one degree-3 multiplicity each)."""
    b = dag.AirBuilder(EP_COLS, aux_width=EP_AUX_COLS, num_randomness=NUM_RANDOMNESS, num_aux_values=NUM_SIGMA_VALUES,
                       num_public=NUM_PUBLIC_VALUES)
    loc, nxt = [b.main(c) for c in range(EP_COLS)], [b.main(c, 1) for c in range(EP_COLS)]
    one = b.const(1)
    is_pai, is_cert, act, act_next = loc[EP_COL_IS_PAI], loc[EP_COL_IS_CERT], loc[EP_COL_ACT], nxt[EP_COL_ACT]
    ptr, ptr_next = loc[EP_COL_PTR], nxt[EP_COL_PTR]
    b.assert_zero(is_pai * (one - is_pai))
    b.assert_zero(is_cert * (one - is_cert))
    b.assert_zero(act * (one - act))
    b.assert_zero(is_pai * is_cert)
    for col in (EP_COL_X_PTR, EP_COL_Y_PTR, EP_COL_U_PTR, EP_COL_W_PTR):  # the point at infinity names no coordinates
        b.assert_zero(is_pai * loc[col])
    for col in (EP_COL_U_PTR, EP_COL_W_PTR):                            # a closure-certified point names no trio
        b.assert_zero(is_cert * loc[col])
    b.assert_zero((one - act) * loc[EP_COL_ECPOINT_MULT])
    b.assert_zero(b.is_transition() * ((one - act) * act_next))
    b.assert_zero(b.is_transition() * (act_next * (ptr_next - ptr - one)))
    b.assert_zero(b.is_first_row() * (ptr - act))

    lk = dag.LogUp(b, MAX_MESSAGE_WIDTH, NUM_BUS_IDS, closing="sigma_last_row")

    def row(ch):
        bb = lk.b if ch is lk.ch_c else lk.lb
        return bb, [bb.main(c) for c in range(EP_COLS)]

    def ec_point(ch):                    # EcPointMsg (ec/mod.rs:122-148)
        _, r = row(ch)
        return ch.encode(BUS_EC_POINT, [r[EP_COL_PTR], r[EP_COL_GROUP_PTR], r[EP_COL_X_PTR], r[EP_COL_Y_PTR], r[EP_COL_IS_PAI]])

    def ec_group(ch):                    # EcGroupMsg (ec/mod.rs:90-116)
        _, r = row(ch)
        return ch.encode(BUS_EC_GROUP, [r[EP_COL_GROUP_PTR], r[EP_COL_A_PTR], r[EP_COL_B_PTR], r[EP_COL_BOUND_PTR], r[EP_COL_SBOUND_PTR]])

    def cert(ch):                        # EcOnCurveCertMsg { group_ptr, r_ptr } (ec/add/mod.rs:169-183)
        _, r = row(ch)
        return ch.encode(BUS_EC_ON_CURVE_CERT, [r[EP_COL_GROUP_PTR], r[EP_COL_PTR]])

    def mac(kappa_c, a_col, b_col, c_col, r_col):     # UintMulMsg (uint/mul/mod.rs:136-170) with kappa_a = 1, is_sub = 0
        def msg(ch):
            bb, r = row(ch)
            return ch.encode(BUS_UINT_MUL, [bb.const(1), bb.const(kappa_c), r[a_col], r[b_col], r[c_col], r[r_col], r[EP_COL_BOUND_PTR],
                                            bb.const(0)])
        return msg

    def mults(fn):
        return fn(lk.b), fn(lk.lb)
    neg_mult = mults(lambda bb: bb.const(0) - bb.main(EP_COL_ECPOINT_MULT))
    m_act = mults(lambda bb: bb.main(EP_COL_ACT))
    m_cert = mults(lambda bb: bb.main(EP_COL_ACT) * bb.main(EP_COL_IS_CERT))
    member = lambda bb: bb.main(EP_COL_ACT) * (bb.const(1) - bb.main(EP_COL_IS_PAI)) * (bb.const(1) - bb.main(EP_COL_IS_CERT))  # noqa: E731
    _emit_frac_cols(lk, [[(neg_mult, ec_point)], [(m_act, ec_group), (m_cert, cert)],
                         [(mults(member), mac(1, EP_COL_X_PTR, EP_COL_X_PTR, EP_COL_A_PTR, EP_COL_U_PTR))],
                         [(mults(member), mac(1, EP_COL_X_PTR, EP_COL_U_PTR, EP_COL_B_PTR, EP_COL_W_PTR))],
                         [(mults(member), mac(0, EP_COL_Y_PTR, EP_COL_Y_PTR, EP_COL_BOUND_PTR, EP_COL_W_PTR))]])
    lookup = lk.finish("ec_point_store")
    return dag.Air(b, _host_aux(lookup, host_aux), "ec_point_store"), lookup


# ---- EcGroupAdd: R = P + Q for any two stored points (ec/add/{mod,trace}.rs, ec/require.rs) ----------------------------------------------
# One four-row block per addition: a near-one-hot over five cases (P at infinity, Q at infinity, cancel, double, generic) whose flags ride
# the consumed `EcPoint` tuples as their `is_pai` fields, and every piece of field arithmetic as a pointer-level certificate consumed from
# the uint relation chiplets -- the chord or tangent slope, x3 = lambda^2 - x1 - x2 and y3 = lambda (x1 - x3) - y1 as scaled
# multiply-subtracts, d = x2 - x1 with its nonzero certificate, y1 + y2 = 0 for the cancel case; no coordinate limb enters this trace.  A
# freshly computed result mints a closure certificate (`EcOnCurveCert`) for its point-store row, under a strict pointer ordering
# r > p, r > q witnessed by Range16 limbs.  21 main columns, twelve flattened LogUp columns on seven buses, four periodic one-hots, lqd 1.
BUS_EC_GROUP_ADD = 16                                                                                           # relations.rs:52-80
EA_COLS, EA_AUX_COLS, EA_PERIOD, EA_NUM_CELLS = 21, 12, 4, 3                                                    # ec/add/mod.rs:190-277
(EA_COL_PX, EA_COL_PY, EA_COL_QX, EA_COL_QY, EA_COL_A_PTR, EA_COL_B_PTR, EA_COL_BOUND_PTR, EA_COL_PAI_P, EA_COL_PAI_Q, EA_COL_CANCEL,
 EA_COL_DBL, EA_COL_GEN, EA_COL_ACT, EA_COL_MINTS, EA_COL_RP_LO, EA_COL_RP_HI, EA_COL_RQ_LO, EA_COL_RQ_HI) = range(3, 21)
EA_ROW_SLOPE, EA_ROW_TAIL, EA_ROW_RES, EA_ROW_TERM = 0, 1, 2, 3
EA_CELL_SLOPE_AUX, EA_CELL_LAMBDA, EA_CELL_T = 0, 1, 2                  # slope row
EA_CELL_Y3, EA_CELL_E, EA_CELL_X3 = 0, 1, 2                             # tail row
EA_CELL_R, EA_CELL_SBOUND, EA_CELL_GROUP = 0, 1, 2                      # res row
EA_TERM_CELL_MULT, EA_TERM_CELL_P, EA_TERM_CELL_Q = 0, 1, 2             # term row


def ec_group_add_air(host_aux=None):
    """`EcGroupAddAir::eval` (ec/add/mod.rs:329-429) and its `LookupAir::eval` (:455-847): col 0 the EcGroupAdd provide | 1 the operands'
    EcPoint consumes | 2 the result's (live / the PAI row of a cancel) | 3 the EcGroup consume + cancel's y1 + y2 = 0 | 4 generic: d, the
    chord | 5 double: the tangent numerator, the slope pin | 6 generic: t, x3 | 7 e, y3 | 8 double: x3 | 9, 10 the ordering limbs | 11 the
    closure-certificate provide."""
    b = dag.AirBuilder(EA_COLS, aux_width=EA_AUX_COLS, num_randomness=NUM_RANDOMNESS, num_aux_values=NUM_SIGMA_VALUES,
                       num_public=NUM_PUBLIC_VALUES, periodic=[[int(r == role) for r in range(EA_PERIOD)] for role in range(EA_PERIOD)])
    loc, nxt = [b.main(c) for c in range(EA_COLS)], [b.main(c, 1) for c in range(EA_COLS)]
    one = b.const(1)
    sel = [b.periodic_value(i) for i in range(EA_PERIOD)]
    pai_p, pai_q, cancel, dbl, generic = (loc[c] for c in (EA_COL_PAI_P, EA_COL_PAI_Q, EA_COL_CANCEL, EA_COL_DBL, EA_COL_GEN))
    act, mints = loc[EA_COL_ACT], loc[EA_COL_MINTS]
    for flag in (pai_p, pai_q, cancel, dbl, generic, act, mints):
        b.assert_zero(flag * (one - flag))
    b.assert_zero(pai_p + pai_q + cancel + dbl + generic - act - pai_p * pai_q)          # one case per live block; both pass flags at PAI + PAI
    b.assert_zero((cancel + dbl) * (loc[EA_COL_PX] - loc[EA_COL_QX]))                     # x1 = x2: pointer equality is value equality
    b.assert_zero(dbl * (loc[EA_COL_PY] - loc[EA_COL_QY]))
    r_cell, p_cell, q_cell = loc[EA_CELL_R], nxt[EA_TERM_CELL_P], nxt[EA_TERM_CELL_Q]
    b.assert_zero(sel[EA_ROW_RES] * pai_p * (r_cell - q_cell))                            # the pass-through ties
    b.assert_zero(sel[EA_ROW_RES] * pai_q * (r_cell - p_cell))
    b.assert_zero(mints * (one - dbl - generic))                                          # only a fresh result mints
    two16 = b.const(1 << 16)
    b.assert_zero(sel[EA_ROW_RES] * mints * (r_cell - p_cell - one - loc[EA_COL_RP_LO] - two16 * loc[EA_COL_RP_HI]))
    b.assert_zero(sel[EA_ROW_RES] * mints * (r_cell - q_cell - one - loc[EA_COL_RQ_LO] - two16 * loc[EA_COL_RQ_HI]))
    not_term = one - sel[EA_ROW_TERM]
    for col in range(EA_COL_PX, EA_COLS):
        b.assert_zero(not_term * (nxt[col] - loc[col]))

    lk = dag.LogUp(b, MAX_MESSAGE_WIDTH, NUM_BUS_IDS, closing="sigma_last_row")

    def win(ch):
        bb = lk.b if ch is lk.ch_c else lk.lb
        return bb, [bb.main(c) for c in range(EA_COLS)], [bb.main(c, 1) for c in range(EA_COLS)]

    def message(bus, fields):            # fields: callables (bb, local, next) -> expression, or plain integers
        def msg(ch):
            bb, lo, nx = win(ch)
            return ch.encode(bus, [bb.const(f) if isinstance(f, int) else f(bb, lo, nx) for f in fields])
        return msg
    L = lambda c: (lambda bb, lo, nx: lo[c])                                              # noqa: E731
    N = lambda c: (lambda bb, lo, nx: nx[c])                                              # noqa: E731
    px, py, qx, qy, a_ptr, bound = L(EA_COL_PX), L(EA_COL_PY), L(EA_COL_QX), L(EA_COL_QY), L(EA_COL_A_PTR), L(EA_COL_BOUND_PTR)
    slope_aux, lam, t = L(EA_CELL_SLOPE_AUX), L(EA_CELL_LAMBDA), L(EA_CELL_T)
    e, x3_next, y3_next = N(EA_CELL_E), N(EA_CELL_X3), N(EA_CELL_Y3)
    group_local, r_local, p_ptr, q_ptr = L(EA_CELL_GROUP), L(EA_CELL_R), N(EA_TERM_CELL_P), N(EA_TERM_CELL_Q)

    def uint_add(a, bb_, c, nz):         # UintAddMsg (uint/add/mod.rs:116-141)
        return message(BUS_UINT_ADD, [bound, a, bb_, c, nz])

    def uint_mul(ka, kc, a, bb_, c, r, is_sub):     # UintMulMsg (uint/mul/mod.rs:136-170)
        return message(BUS_UINT_MUL, [ka, kc, a, bb_, c, r, bound, is_sub])

    def ec_point(ptr, group, x, y, is_pai):         # EcPointMsg (ec/mod.rs:122-148)
        return message(BUS_EC_POINT, [ptr, group, x, y, is_pai])

    def mults(fn):
        return fn(lk.b), fn(lk.lb)

    def gate(row, cols, neg=False):      # (sum of the flag columns) * the row's one-hot
        def fn(bb):
            acc = bb.main(cols[0])
            for c in cols[1:]:
                acc = acc + bb.main(c)
            acc = acc * bb.periodic_value(row)
            return bb.const(0) - acc if neg else acc
        return mults(fn)
    at_res_act = gate(EA_ROW_RES, [EA_COL_ACT])
    at_slope_gen, at_slope_dbl = gate(EA_ROW_SLOPE, [EA_COL_GEN]), gate(EA_ROW_SLOPE, [EA_COL_DBL])
    at_slope_tail = gate(EA_ROW_SLOPE, [EA_COL_DBL, EA_COL_GEN])
    at_res_cancel = gate(EA_ROW_RES, [EA_COL_CANCEL])
    at_res_mints = mults(lambda bb: bb.periodic_value(EA_ROW_RES) * bb.main(EA_COL_MINTS))
    neg_res_mints = mults(lambda bb: bb.const(0) - bb.periodic_value(EA_ROW_RES) * bb.main(EA_COL_MINTS))
    provide = mults(lambda bb: (bb.const(0) - bb.main(EA_TERM_CELL_MULT, 1)) * bb.periodic_value(EA_ROW_RES))
    range16 = lambda c: message(BUS_RANGE16, [L(c)])                                      # noqa: E731
    _emit_frac_cols(lk, [
        [(provide, message(BUS_EC_GROUP_ADD, [group_local, p_ptr, q_ptr, r_local]))],
        [(at_res_act, ec_point(p_ptr, group_local, px, py, L(EA_COL_PAI_P))), (at_res_act, ec_point(q_ptr, group_local, qx, qy, L(EA_COL_PAI_Q)))],
        [(gate(EA_ROW_TAIL, [EA_COL_DBL, EA_COL_GEN]), ec_point(N(EA_CELL_R), N(EA_CELL_GROUP), L(EA_CELL_X3), L(EA_CELL_Y3), 0)),
         (at_res_cancel, ec_point(r_local, group_local, 0, 0, 1))],
        [(gate(EA_ROW_RES, [EA_COL_CANCEL, EA_COL_DBL, EA_COL_GEN]),
          message(BUS_EC_GROUP, [group_local, a_ptr, L(EA_COL_B_PTR), bound, L(EA_CELL_SBOUND)])),
         (at_res_cancel, uint_add(py, qy, 0, 0))],
        [(at_slope_gen, uint_add(px, slope_aux, qx, 1)), (at_slope_gen, uint_mul(1, 1, lam, slope_aux, py, qy, 0))],
        [(at_slope_dbl, uint_mul(3, 1, px, px, a_ptr, slope_aux, 0)), (at_slope_dbl, uint_mul(2, 0, lam, py, bound, slope_aux, 0))],
        [(at_slope_gen, uint_add(px, qx, t, 0)), (at_slope_gen, uint_mul(1, 1, lam, lam, t, x3_next, 1))],
        [(at_slope_tail, uint_add(x3_next, e, px, 0)), (at_slope_tail, uint_mul(1, 1, lam, e, py, y3_next, 1))],
        [(at_slope_dbl, uint_mul(1, 2, lam, lam, px, x3_next, 1))],
        [(at_res_mints, range16(EA_COL_RP_LO)), (at_res_mints, range16(EA_COL_RP_HI))],
        [(at_res_mints, range16(EA_COL_RQ_LO)), (at_res_mints, range16(EA_COL_RQ_HI))],
        [(neg_res_mints, message(BUS_EC_ON_CURVE_CERT, [group_local, r_local]))]])
    lookup = lk.finish("ec_group_add")
    return dag.Air(b, _host_aux(lookup, host_aux), "ec_group_add"), lookup


# ---- UintStoreMul: the uint store and the scaled multiply-accumulate relation on one row range (uint/{mod,trace}.rs, uint/mul/{mod,trace}.rs,
# uint/store_mul/{mod,trace}.rs) ------------------------------------------------------------------------------------------------------------
# STORE (main columns 0..18, period 4): one block per stored 256-bit value -- v as sixteen Range16-checked 16-bit limbs on two rows, its
# complement to the bound (comp = bound - v: the range check v <= bound) on a third, the bound as 4 x 32 + 4 x 32 bits with seven binary
# carries and the pointer gap on the closing row.  v + comp = bound is checked by a vertical Schwartz-Zippel: an extension-field REGISTER
# `id` in the aux trace accumulates the rows' limb sums at the LogUp challenge beta and must return to zero at every block end.  Provides
# the value as `UintVal` (8 x 32) and `UintLimbs` (16 x 16); consumes its own bound's `UintVal` (only a self-referential row -- a modulus --
# can answer that).  MUL (columns 18..44, period 8): kappa_a a b +- kappa_c c = r (mod bound + 1) over stored values: a, b, the bound as
# 16-bit limb rows (pulled over `UintLimbs`), a 17-limb quotient, r and c as 32-bit rows (`UintVal`), 31 carry coefficients in 62
# offset 16-bit halves spread over the free cells (`UM_GAMMA_SLOTS`); the identity
#     kappa_a a(beta) b(beta) +- kappa_c C(beta^2) - q(beta) (bound(beta) + 1) - R(beta^2) + (beta - 2^16) Gamma(beta) = 0
# again by registers: `S` stages kappa_a a(beta), then bound(beta) (a periodic keep gate), `id` accumulates S b(beta), -(S + 1) q(beta)
# and the linear terms.  44 main columns, 26 LogUp columns + 3 registers, 13 periodic columns, lqd 1.
BUS_UINT_LIMBS = 13                                                                                             # relations.rs:52-80
US_CELLS, US_COL_PTR, US_COL_BOUND_PTR, US_COLS, US_PERIOD = 16, 16, 17, 18, 4                                  # uint/mod.rs:180-196
US_HUB_UINTVAL_MULT, US_HUB_UINTLIMBS_MULT, US_CARRY_LO, US_CARRY_HI, US_TERM_GAP = 8, 9, 4, 12, 15
UM_CELLS, UM_COLS, UM_PERIOD = 19, 26, 8                                                                        # uint/mul/mod.rs:175-206
UM_COL_A_PTR, UM_COL_B_PTR, UM_COL_R_PTR, UM_COL_BOUND_PTR, UM_COL_KAPPA_A, UM_COL_ACT, UM_COL_BORROW = range(19, 26)
UM_ROW_A, UM_ROW_B, UM_ROW_P, UM_ROW_Q, UM_ROW_R, UM_ROW_G0, UM_ROW_G1, UM_ROW_C = range(8)
UM_S_KEEP = [1, 0, 1, 0, 0, 0, 0, 0]
UM_TERM_MULT, UM_TERM_C_PTR, UM_TERM_KAPPA_C, UM_TERM_IS_SUB, UM_TERM_KAPPA_C_SIGNED = 8, 9, 10, 11, 12        # on the c row (:212-216)
UM_NUM_Q_LIMBS, UM_NUM_GAMMA, UM_GAMMA_OFFSET = 17, 31, 1 << 31                                                 # :218-219, :346
UM_GAMMA_SLOTS = ([(UM_ROW_G0, c) for c in range(19)] + [(UM_ROW_G1, c) for c in range(15)]                     # `gamma_slots` (:225-282)
                  + [(r, c) for r in (UM_ROW_A, UM_ROW_B, UM_ROW_P) for c in range(16, 19)] + [(UM_ROW_Q, c) for c in range(17, 19)]
                  + [(UM_ROW_R, c) for c in range(8, 19)] + [(UM_ROW_C, c) for c in range(13, 19)])
USM_MUL_OFF, USM_COLS = US_COLS, US_COLS + UM_COLS                                                              # uint/store_mul/mod.rs:76-101
USM_STORE_LOGUP_COLS, USM_MUL_LOGUP_COLS = 1 + 1 + 8 + 1, 1 + 2 + 10 + 1 + 1
USM_LOGUP_COLS = USM_STORE_LOGUP_COLS + USM_MUL_LOGUP_COLS
USM_STORE_REG_ID, USM_MUL_REG_ID, USM_MUL_REG_S, USM_AUX_COLS = USM_LOGUP_COLS, USM_LOGUP_COLS + 1, USM_LOGUP_COLS + 2, USM_LOGUP_COLS + 3
USM_PCOL_S_KEEP, USM_PCOL_STORE_ROLE = UM_PERIOD, UM_PERIOD + 1        # periodic: mul's eight one-hots, S_KEEP, the store's four roles tiled twice
assert len(UM_GAMMA_SLOTS) == 2 * UM_NUM_GAMMA == len(set(UM_GAMMA_SLOTS))


def _usm_periodic():
    cols = [[int(r == role) for r in range(UM_PERIOD)] for role in range(UM_PERIOD)]
    cols.append(list(UM_S_KEEP))
    cols += [[int(r % US_PERIOD == role) for r in range(UM_PERIOD)] for role in range(US_PERIOD)]
    return cols


def _usm_store_parts(bb):
    """The store's `id` contribution of a row and the closing row's own share (uint/store_mul/mod.rs:197-302), on builder `bb`."""
    loc = [bb.main(c) for c in range(US_COLS)]
    v_lo, v_hi, comp, bound = (bb.periodic_value(USM_PCOL_STORE_ROLE + k) for k in range(4))
    beta = bb.randomness(1)
    bp = [bb.const(1)]
    for _ in range(1, 8):
        bp.append(bp[-1] * beta)
    two16, t32 = bb.const(1 << 16), bb.const(1 << 32)
    zero = bb.const(0)
    lo07 = hi07 = hi815 = direct_lo = direct_hi = zero
    for k in range(4):
        r07, r815 = loc[2 * k] + two16 * loc[2 * k + 1], loc[8 + 2 * k] + two16 * loc[8 + 2 * k + 1]
        lo07, hi07, hi815 = lo07 + bp[k] * r07, hi07 + bp[4 + k] * r07, hi815 + bp[4 + k] * r815
        direct_lo, direct_hi = direct_lo + bp[k] * loc[k], direct_hi + bp[4 + k] * loc[8 + k]
    carry_lo = carry_hi = zero
    for j in range(4):
        carry_lo = carry_lo + (bp[j + 1] - bp[j] * t32) * loc[US_CARRY_LO + j]
    for j in range(4, 7):
        carry_hi = carry_hi + (bp[j + 1] - bp[j] * t32) * loc[US_CARRY_HI + (j - 4)]
    bound_own = carry_lo - direct_lo + carry_hi - direct_hi
    contrib = lo07 * (v_lo + comp) + hi07 * v_hi + hi815 * comp + bound_own * bound
    return contrib, bound_own, bound


def _usm_mul_parts(bb):
    """The multiplier's registers on builder `bb` (uint/store_mul/mod.rs:304-440): S' = keep S + build, id' = id + S u + v, and the c row's
    own share of the closing check."""
    loc = [bb.main(USM_MUL_OFF + c) for c in range(UM_COLS)]
    sel = [bb.periodic_value(i) for i in range(UM_PERIOD)]
    keep = bb.periodic_value(USM_PCOL_S_KEEP)
    beta = bb.randomness(1)
    bp = [bb.const(1)]
    for _ in range(1, UM_NUM_GAMMA + 1):
        bp.append(bp[-1] * beta)
    t16, offset, one = bb.const(1 << 16), bb.const(UM_GAMMA_OFFSET), bb.const(1)
    x_minus_t = beta - t16
    kappa_a, act, borrow, kcs = loc[UM_COL_KAPPA_A], loc[UM_COL_ACT], loc[UM_COL_BORROW], loc[UM_TERM_KAPPA_C_SIGNED]
    full16 = full_q = val = bb.const(0)
    for i_ in range(UM_NUM_Q_LIMBS):
        if i_ < 16:
            full16 = full16 + bp[i_] * loc[i_]
        full_q = full_q + bp[i_] * loc[i_]
    for m in range(8):
        val = val + bp[2 * m] * loc[m]
    build = full16 * (sel[UM_ROW_A] * kappa_a) + full16 * sel[UM_ROW_P]
    u = full16 * sel[UM_ROW_B] - full_q * sel[UM_ROW_Q]
    carries, c_own = bb.const(0), val * kcs
    for slot, (row, cell) in enumerate(UM_GAMMA_SLOTS):
        w = x_minus_t * bp[slot // 2]
        if slot % 2:
            w = w * t16
        gated = sel[row] * loc[cell]
        own = loc[cell]
        if slot % 2 == 0:
            gated, own = gated - sel[row] * act * offset, own - act * offset
        carries = carries + w * gated
        if row == UM_ROW_C:
            c_own = c_own + w * own
    v = val * (sel[UM_ROW_C] * kcs) - val * sel[UM_ROW_R] - full_q * sel[UM_ROW_Q] + carries + (full16 + one) * (sel[UM_ROW_P] * borrow)
    return dict(keep=keep, build=build, u=u, v=v, c_own=c_own, loc=loc, sel=sel)


def uint_store_mul_air(host_aux=None):
    """`UintStoreMulAir::eval` (uint/store_mul/mod.rs:196-446: the store's and the multiplier's constraints verbatim, side by side) and its
    `LookupAir::eval` (:471-889): cols 0-10 the store's (UintVal provide | its bound's consume + the gap | eight Range16 pairs | UintLimbs
    provide), cols 11-25 the multiplier's (UintMul provide | three UintLimbs consumes | ten Range16 columns over the 19 cells | the two
    kappas | the r and c UintVal consumes); aux columns 26-28 = the registers (store id, mul id, mul S), built by the lookup program's
    register tail (`dag.LogUp.register`)."""
    b = dag.AirBuilder(USM_COLS, aux_width=USM_AUX_COLS, num_randomness=NUM_RANDOMNESS, num_aux_values=NUM_SIGMA_VALUES,
                       num_public=NUM_PUBLIC_VALUES, periodic=_usm_periodic())
    one = b.const(1)
    # ---- store
    loc, nxt = [b.main(c) for c in range(US_COLS)], [b.main(c, 1) for c in range(US_COLS)]
    contrib, bound_own, bound_sel = _usm_store_parts(b)
    sid, sid_next = b.aux(USM_STORE_REG_ID), b.aux(USM_STORE_REG_ID, 1)
    b.assert_zero_ext(b.is_first_row() * sid)
    b.assert_zero_ext(b.is_transition() * (sid_next - sid - contrib))
    b.assert_zero_ext((sid + bound_own) * bound_sel)
    b.assert_zero(b.is_first_row() * (loc[US_COL_PTR] - one))           # the pointer chain is rooted at 1: 0 stays the unstored sentinel
    for cell in list(range(US_CARRY_LO, US_CARRY_LO + 4)) + list(range(US_CARRY_HI, US_CARRY_HI + 3)):
        b.assert_zero(bound_sel * loc[cell] * (one - loc[cell]))
    not_term = one - bound_sel
    for col in (US_COL_PTR, US_COL_BOUND_PTR):
        b.assert_zero(not_term * (nxt[col] - loc[col]))
    b.assert_zero(b.is_transition() * (bound_sel * (loc[US_TERM_GAP] + loc[US_COL_PTR] + one - nxt[US_COL_PTR])))
    # ---- mul
    m = _usm_mul_parts(b)
    ml, mn, sel = m["loc"], [b.main(USM_MUL_OFF + c, 1) for c in range(UM_COLS)], m["sel"]
    mid, mid_next, s_reg, s_next = b.aux(USM_MUL_REG_ID), b.aux(USM_MUL_REG_ID, 1), b.aux(USM_MUL_REG_S), b.aux(USM_MUL_REG_S, 1)
    b.assert_zero_ext(b.is_first_row() * s_reg)
    b.assert_zero_ext(b.is_transition() * (s_next - s_reg * m["keep"] - m["build"]))
    b.assert_zero_ext(b.is_first_row() * mid)
    b.assert_zero_ext(b.is_transition() * (mid_next - mid - (s_reg * m["u"] + m["v"])))
    b.assert_zero_ext((mid + m["c_own"]) * sel[UM_ROW_C])
    act, borrow, is_sub = ml[UM_COL_ACT], ml[UM_COL_BORROW], ml[UM_TERM_IS_SUB]
    b.assert_zero(act * (one - act))
    b.assert_zero(sel[UM_ROW_C] * is_sub * (one - is_sub))
    b.assert_zero(sel[UM_ROW_C] * (ml[UM_TERM_KAPPA_C_SIGNED] - ml[UM_TERM_KAPPA_C] * (one - b.const(2) * is_sub)))
    b.assert_zero(borrow * (borrow - one) * (borrow - b.const(2)))
    b.assert_zero(sel[UM_ROW_C] * borrow * (one - is_sub))
    b.assert_zero(sel[UM_ROW_C] * (one - act) * ml[UM_TERM_MULT])
    m_not_term = one - sel[UM_ROW_C]
    for col in (UM_COL_A_PTR, UM_COL_B_PTR, UM_COL_R_PTR, UM_COL_BOUND_PTR, UM_COL_KAPPA_A, UM_COL_ACT, UM_COL_BORROW):
        b.assert_zero(m_not_term * (mn[col] - ml[col]))

    lk = dag.LogUp(b, MAX_MESSAGE_WIDTH, NUM_BUS_IDS, closing="sigma_last_row", num_logup_cols=USM_LOGUP_COLS)

    def win(ch):
        bb = lk.b if ch is lk.ch_c else lk.lb
        return bb, [bb.main(c) for c in range(USM_COLS)], [bb.main(c, 1) for c in range(USM_COLS)]

    def message(bus, fields):            # fields: callables (bb, local, next) -> expression
        def msg(ch):
            bb, lo, nx = win(ch)
            return ch.encode(bus, [f(bb, lo, nx) for f in fields])
        return msg
    L = lambda c: (lambda bb, lo, nx: lo[c])                                              # noqa: E731
    N = lambda c: (lambda bb, lo, nx: nx[c])                                              # noqa: E731
    recomb = [(lambda k: (lambda bb, lo, nx: (lo if k < 4 else nx)[2 * (k % 4)] + bb.const(1 << 16) * (lo if k < 4 else nx)[2 * (k % 4) + 1]))(k)
              for k in range(8)]
    direct = [L(k) if k < 4 else L(4 + k) for k in range(8)]
    raw = [L(j) if j < 8 else N(j - 8) for j in range(16)]
    M = USM_MUL_OFF

    def mults(fn):
        return fn(lk.b), fn(lk.lb)
    role = lambda bb, k: bb.periodic_value(USM_PCOL_STORE_ROLE + k)                       # noqa: E731
    limb_gate = lambda cell: mults(lambda bb: role(bb, 0) + role(bb, 1) + role(bb, 2) if cell < 8 else role(bb, 2))   # noqa: E731
    bound_gate = mults(lambda bb: role(bb, 3))
    columns = [[(mults(lambda bb: (bb.const(0) - bb.main(US_HUB_UINTVAL_MULT, 1)) * role(bb, 0)),
                 message(BUS_UINT_VAL, [L(US_COL_PTR), L(US_COL_BOUND_PTR)] + recomb))],
               [(bound_gate, message(BUS_UINT_VAL, [L(US_COL_BOUND_PTR), L(US_COL_BOUND_PTR)] + direct)),
                (bound_gate, message(BUS_RANGE16, [L(US_TERM_GAP)]))]]
    for cell in range(0, US_CELLS, 2):
        columns.append([(limb_gate(c), message(BUS_RANGE16, [L(c)])) for c in (cell, cell + 1)])
    columns.append([(mults(lambda bb: (bb.const(0) - bb.main(US_HUB_UINTLIMBS_MULT, 1)) * role(bb, 0)),
                     message(BUS_UINT_LIMBS, [L(US_COL_PTR), L(US_COL_BOUND_PTR)] + raw))])
    # the multiplier's columns
    row_act = lambda row: mults(lambda bb: bb.periodic_value(row) * bb.main(M + UM_COL_ACT))           # noqa: E731
    columns.append([(mults(lambda bb: (bb.const(0) - bb.main(M + UM_TERM_MULT)) * bb.periodic_value(UM_ROW_C)),
                     message(BUS_UINT_MUL, [L(M + UM_COL_KAPPA_A), L(M + UM_TERM_KAPPA_C), L(M + UM_COL_A_PTR), L(M + UM_COL_B_PTR), L(M + UM_TERM_C_PTR),
                                            L(M + UM_COL_R_PTR), L(M + UM_COL_BOUND_PTR), L(M + UM_TERM_IS_SUB)]))])
    limbs16 = [L(M + i_) for i_ in range(16)]
    raw_consumes = [(row_act(row), message(BUS_UINT_LIMBS, [L(M + ptr), L(M + UM_COL_BOUND_PTR)] + limbs16))
                    for row, ptr in ((UM_ROW_A, UM_COL_A_PTR), (UM_ROW_B, UM_COL_B_PTR), (UM_ROW_P, UM_COL_BOUND_PTR))]
    columns += [raw_consumes[0:2], raw_consumes[2:3]]

    def cell_gate(cell):
        rows = ([UM_ROW_Q] if cell < UM_NUM_Q_LIMBS else []) + [r for r, c in UM_GAMMA_SLOTS if c == cell]

        def fn(bb):
            acc = bb.periodic_value(rows[0])
            for r in rows[1:]:
                acc = acc + bb.periodic_value(r)
            return acc * bb.main(M + UM_COL_ACT)
        return mults(fn)
    cells = [(cell_gate(c), message(BUS_RANGE16, [L(M + c)])) for c in range(UM_CELLS)]
    columns += [cells[c:c + 2] for c in range(0, UM_CELLS, 2)]
    columns.append([(row_act(UM_ROW_C), message(BUS_RANGE16, [L(M + UM_COL_KAPPA_A)])), (row_act(UM_ROW_C), message(BUS_RANGE16, [L(M + UM_TERM_KAPPA_C)]))])
    val_full = [L(M + i_) for i_ in range(8)]
    columns.append([(row_act(UM_ROW_R), message(BUS_UINT_VAL, [L(M + UM_COL_R_PTR), L(M + UM_COL_BOUND_PTR)] + val_full)),
                    (row_act(UM_ROW_C), message(BUS_UINT_VAL, [L(M + UM_TERM_C_PTR), L(M + UM_COL_BOUND_PTR)] + val_full))])
    assert len(columns) == USM_LOGUP_COLS
    _emit_frac_cols(lk, columns)
    parts = _usm_mul_parts(lk.lb)
    assert lk.register(None, lambda bb: _usm_store_parts(bb)[0]) == USM_STORE_REG_ID
    assert lk.register(None, lambda bb: parts["v"], [(USM_MUL_REG_S, lambda bb: parts["u"])]) == USM_MUL_REG_ID     # id reads S, the column after it
    assert lk.register(lambda bb: parts["keep"], lambda bb: parts["build"]) == USM_MUL_REG_S
    lookup = lk.finish("uint_store_mul")
    return dag.Air(b, _host_aux(lookup, host_aux), "uint_store_mul"), lookup


# ---- EcMsm: symbolic multi-scalar-multiplication expressions (ec/msm/{mod,trace,require}.rs) --------------------------------------------
# A term = (base point, scalar) "P x s"; an expression = a run of term rows sharing one `expr_ptr`, with a value point `val` and the
# invariant deref(val) = sum of s P.  Three rules build any addition chain: `intro` (<P x 1>, val = P), `neg` (every scalar negated,
# val = -val_a as a trio-free certified point), `combine` (the two sorted term lists merged, scalars on a shared base added mod the scalar
# bound, values added by a consumed `EcGroupAdd`).  The AIR checks that each step is sound, never which steps were taken: variable-length
# blocks (the allocator chain expr_ptr' = expr_ptr + is_boundary), merge-walk cursors i, j over the operands' `MsmTerm` tuples, a strict
# pointer ordering a_expr, b_expr < expr against circular derivations.  38 main columns, eleven flattened LogUp columns on nine buses, lqd 1.
BUS_MSM_TERM, BUS_MSM_EXPR, BUS_MSM_CLAIM_TERM = 18, 19, 20                                                     # relations.rs:52-80
MS_COLS, MS_AUX_COLS = 38, 11                                                                                   # ec/msm/mod.rs:157-273
(MS_COL_ACT, MS_COL_EXPR_PTR, MS_COL_IS_BOUNDARY, MS_COL_GROUP_PTR, MS_COL_SBOUND_PTR, MS_COL_IDX, MS_COL_BASE, MS_COL_SCALAR, MS_COL_VAL,
 MS_COL_MULT, MS_COL_IS_INTRO, MS_COL_IS_COMBINE, MS_COL_A_EXPR, MS_COL_B_EXPR, MS_COL_I, MS_COL_J, MS_COL_TAKE_A, MS_COL_TAKE_B,
 MS_COL_TAKE_BOTH, MS_COL_BASE_A, MS_COL_S_A, MS_COL_BASE_B, MS_COL_S_B, MS_COL_VAL_A, MS_COL_VAL_B, MS_COL_A_PTR, MS_COL_B_PTR,
 MS_COL_BOUND_PTR, MS_COL_A_DIFF_LO, MS_COL_A_DIFF_HI, MS_COL_B_DIFF_LO, MS_COL_B_DIFF_HI, MS_COL_IS_NEG, MS_COL_NEG_X, MS_COL_CLAIM_MULT,
 MS_COL_NEG_YA, MS_COL_NEG_YR, MS_COL_NEG_MINTED) = range(38)


def ec_msm_air(host_aux=None):
    """`EcMsmAir::eval` (ec/msm/mod.rs:316-488) and its `LookupAir::eval` (:510-856): col 0 the MsmTerm provide | 1 the MsmExpr head + the
    positionless MsmClaimTerm provides | 2 neg's closure certificate + intro's literal-1 scalar | 3 the walk's A term | 4 its B term + the
    merged scalar | 5 neg's scalar and y flips | 6 the operands' heads | 7 combine's value addition + neg's operand point | 8 neg's result
    point + the group | 9, 10 the ordering limbs."""
    b = dag.AirBuilder(MS_COLS, aux_width=MS_AUX_COLS, num_randomness=NUM_RANDOMNESS, num_aux_values=NUM_SIGMA_VALUES,
                       num_public=NUM_PUBLIC_VALUES)
    loc, nxt = [b.main(c) for c in range(MS_COLS)], [b.main(c, 1) for c in range(MS_COLS)]
    one = b.const(1)
    act, act_next, is_boundary = loc[MS_COL_ACT], nxt[MS_COL_ACT], loc[MS_COL_IS_BOUNDARY]
    is_intro, is_combine, is_neg, neg_minted, idx = loc[MS_COL_IS_INTRO], loc[MS_COL_IS_COMBINE], loc[MS_COL_IS_NEG], loc[MS_COL_NEG_MINTED], loc[MS_COL_IDX]
    tr = b.is_transition()
    for col in (MS_COL_ACT, MS_COL_IS_BOUNDARY, MS_COL_IS_INTRO, MS_COL_IS_COMBINE, MS_COL_IS_NEG, MS_COL_NEG_MINTED):
        _assert_bool(b, loc[col])
    b.assert_zero((one - is_neg) * neg_minted)
    b.assert_zero(tr * ((one - act) * act_next))
    b.assert_zero(is_intro + is_combine + is_neg - act)
    b.assert_zero((one - act) * is_boundary)
    b.assert_zero((one - act) * loc[MS_COL_MULT])
    b.assert_zero((one - act) * loc[MS_COL_CLAIM_MULT])
    b.assert_zero(b.is_first_row() * (loc[MS_COL_EXPR_PTR] - one))       # the allocator: pointers are run numbers
    b.assert_zero(tr * (nxt[MS_COL_EXPR_PTR] - loc[MS_COL_EXPR_PTR] - is_boundary))
    b.assert_zero(b.is_first_row() * idx)
    b.assert_zero(tr * (nxt[MS_COL_IDX] - (one - is_boundary) * (idx + one)))
    not_boundary = one - is_boundary
    for col in (MS_COL_GROUP_PTR, MS_COL_SBOUND_PTR, MS_COL_VAL, MS_COL_MULT, MS_COL_CLAIM_MULT, MS_COL_IS_INTRO, MS_COL_IS_COMBINE, MS_COL_IS_NEG,
                MS_COL_A_EXPR, MS_COL_B_EXPR, MS_COL_VAL_A, MS_COL_VAL_B, MS_COL_A_PTR, MS_COL_B_PTR, MS_COL_BOUND_PTR):
        b.assert_zero(tr * (not_boundary * (nxt[col] - loc[col])))
    b.assert_zero(is_intro * (one - is_boundary))
    b.assert_zero(is_intro * (loc[MS_COL_VAL] - loc[MS_COL_BASE]))
    take_a, take_b, take_both = loc[MS_COL_TAKE_A], loc[MS_COL_TAKE_B], loc[MS_COL_TAKE_BOTH]
    for t in (take_a, take_b, take_both):
        _assert_bool(b, t)
    b.assert_zero(take_a + take_b + take_both - is_combine)
    i_cur, j_cur = loc[MS_COL_I], loc[MS_COL_J]
    b.assert_zero(b.is_first_row() * i_cur)
    b.assert_zero(b.is_first_row() * j_cur)
    adv_i, adv_j = take_a + take_both + is_neg, take_b + take_both
    b.assert_zero(tr * (nxt[MS_COL_I] - (one - is_boundary) * (i_cur + adv_i)))
    b.assert_zero(tr * (nxt[MS_COL_J] - (one - is_boundary) * (j_cur + adv_j)))
    base_a, base_b, s_a, s_b = loc[MS_COL_BASE_A], loc[MS_COL_BASE_B], loc[MS_COL_S_A], loc[MS_COL_S_B]
    b.assert_zero((take_a + take_both + is_neg) * (loc[MS_COL_BASE] - base_a) + take_b * (loc[MS_COL_BASE] - base_b))
    b.assert_zero(take_a * (loc[MS_COL_SCALAR] - s_a) + take_b * (loc[MS_COL_SCALAR] - s_b))
    b.assert_zero(take_both * (base_a - base_b))
    two16 = b.const(1 << 16)
    b.assert_zero((is_combine + is_neg) * is_boundary * (loc[MS_COL_EXPR_PTR] - loc[MS_COL_A_EXPR] - one - loc[MS_COL_A_DIFF_LO] - two16 * loc[MS_COL_A_DIFF_HI]))
    b.assert_zero(is_combine * is_boundary * (loc[MS_COL_EXPR_PTR] - loc[MS_COL_B_EXPR] - one - loc[MS_COL_B_DIFF_LO] - two16 * loc[MS_COL_B_DIFF_HI]))

    lk = dag.LogUp(b, MAX_MESSAGE_WIDTH, NUM_BUS_IDS, closing="sigma_last_row")

    def message(bus, fields):            # fields: column numbers, callables bb -> expression, or ("const", value)
        def msg(ch):
            bb = lk.b if ch is lk.ch_c else lk.lb
            return ch.encode(bus, [bb.main(f) if isinstance(f, int) else (bb.const(f[1]) if isinstance(f, tuple) else f(bb)) for f in fields])
        return msg
    K = lambda v: ("const", v)                                                            # noqa: E731

    def mults(fn):
        return fn(lk.b), fn(lk.lb)
    m = lambda c: (lambda bb: bb.main(c))                                                 # noqa: E731
    f_adv_i = lambda bb: bb.main(MS_COL_TAKE_A) + bb.main(MS_COL_TAKE_BOTH) + bb.main(MS_COL_IS_NEG)          # noqa: E731
    f_adv_j = lambda bb: bb.main(MS_COL_TAKE_B) + bb.main(MS_COL_TAKE_BOTH)                                   # noqa: E731
    bnd_a = mults(lambda bb: (bb.main(MS_COL_IS_COMBINE) + bb.main(MS_COL_IS_NEG)) * bb.main(MS_COL_IS_BOUNDARY))
    bnd_b = mults(lambda bb: bb.main(MS_COL_IS_COMBINE) * bb.main(MS_COL_IS_BOUNDARY))
    bnd_neg = mults(lambda bb: bb.main(MS_COL_IS_NEG) * bb.main(MS_COL_IS_BOUNDARY))
    neg_mult = mults(lambda bb: bb.const(0) - bb.main(MS_COL_MULT))
    neg_claim = mults(lambda bb: bb.const(0) - bb.main(MS_COL_CLAIM_MULT))
    ec_point = lambda ptr, y: message(BUS_EC_POINT, [ptr, MS_COL_GROUP_PTR, MS_COL_NEG_X, y, K(0)])           # noqa: E731
    _emit_frac_cols(lk, [
        [(neg_mult, message(BUS_MSM_TERM, [MS_COL_EXPR_PTR, MS_COL_IDX, MS_COL_BASE, MS_COL_SCALAR]))],
        [(mults(lambda bb: (bb.const(0) - bb.main(MS_COL_MULT) + (bb.const(0) - bb.main(MS_COL_CLAIM_MULT))) * bb.main(MS_COL_IS_BOUNDARY)),
          message(BUS_MSM_EXPR, [MS_COL_EXPR_PTR, MS_COL_GROUP_PTR, MS_COL_VAL, lambda bb: bb.main(MS_COL_IDX) + bb.const(1)])),
         (neg_claim, message(BUS_MSM_CLAIM_TERM, [MS_COL_EXPR_PTR, MS_COL_BASE, MS_COL_SCALAR]))],
        [(mults(lambda bb: bb.const(0) - bb.main(MS_COL_NEG_MINTED) * bb.main(MS_COL_IS_BOUNDARY)), message(BUS_EC_ON_CURVE_CERT, [MS_COL_GROUP_PTR, MS_COL_VAL])),
         (mults(m(MS_COL_IS_INTRO)), message(BUS_UINT_VAL, [MS_COL_SCALAR, MS_COL_SBOUND_PTR, K(1)] + [K(0)] * 7))],
        [(mults(f_adv_i), message(BUS_MSM_TERM, [MS_COL_A_EXPR, MS_COL_I, MS_COL_BASE_A, MS_COL_S_A]))],
        [(mults(f_adv_j), message(BUS_MSM_TERM, [MS_COL_B_EXPR, MS_COL_J, MS_COL_BASE_B, MS_COL_S_B])),
         (mults(m(MS_COL_TAKE_BOTH)), message(BUS_UINT_ADD, [MS_COL_SBOUND_PTR, MS_COL_S_A, MS_COL_S_B, MS_COL_SCALAR, K(0)]))],
        [(mults(m(MS_COL_IS_NEG)), message(BUS_UINT_ADD, [MS_COL_SBOUND_PTR, MS_COL_S_A, MS_COL_SCALAR, K(0), K(0)])),
         (bnd_neg, message(BUS_UINT_ADD, [MS_COL_BOUND_PTR, MS_COL_NEG_YA, MS_COL_NEG_YR, K(0), K(0)]))],
        [(bnd_a, message(BUS_MSM_EXPR, [MS_COL_A_EXPR, MS_COL_GROUP_PTR, MS_COL_VAL_A, lambda bb: bb.main(MS_COL_I) + f_adv_i(bb)])),
         (bnd_b, message(BUS_MSM_EXPR, [MS_COL_B_EXPR, MS_COL_GROUP_PTR, MS_COL_VAL_B, lambda bb: bb.main(MS_COL_J) + f_adv_j(bb)]))],
        [(bnd_b, message(BUS_EC_GROUP_ADD, [MS_COL_GROUP_PTR, MS_COL_VAL_A, MS_COL_VAL_B, MS_COL_VAL])), (bnd_neg, ec_point(MS_COL_VAL_A, MS_COL_NEG_YA))],
        [(bnd_neg, ec_point(MS_COL_VAL, MS_COL_NEG_YR)),
         (bnd_a, message(BUS_EC_GROUP, [MS_COL_GROUP_PTR, MS_COL_A_PTR, MS_COL_B_PTR, MS_COL_BOUND_PTR, MS_COL_SBOUND_PTR]))],
        [(bnd_a, message(BUS_RANGE16, [MS_COL_A_DIFF_LO])), (bnd_a, message(BUS_RANGE16, [MS_COL_A_DIFF_HI]))],
        [(bnd_b, message(BUS_RANGE16, [MS_COL_B_DIFF_LO])), (bnd_b, message(BUS_RANGE16, [MS_COL_B_DIFF_HI]))]])
    lookup = lk.finish("ec_msm")
    return dag.Air(b, _host_aux(lookup, host_aux), "ec_msm"), lookup


def _assert_bool(b, x):                  # p3's `assert_bool`: x (x - 1)
    b.assert_zero(x * (x - b.const(1)))


# ---- TranscriptEval: the transcript's hasher and binder (transcript/eval/{mod,trace}.rs, transcript/{binding,nodes}.rs, poseidon2/digest.rs) --
# One node of the transcript DAG per active row: it hashes the node's preimage on the Poseidon2 chiplet (`lhs || rhs` under a capacity
# that names the node kind) and settles the node's `Binding` tuple.  Kinds, a one-hot over the active row: the AND combinator folding two
# `True` bindings (the root on row 0: its hash IS the public input), the ZERO_HASH leaf, uint leaves (a stored value under the VM's VALUE
# capacity, or an explicit pin claim folded into the spine), uint ops (add / sub / mul bind the result pointer as a `Uint` binding and
# consume the relation tuple that wires the pointers; `is` binds True), EC create / point at infinity, EC ops, and the one multi-row node,
# an EcMsm absorb run (one Poseidon2 absorption span over the claim's (point, scalar) child digests, its terms matched as a positionless
# set against the MSM chiplet).  All value soundness lives at the relation chiplets and stores; this chip is hashing and pointer wiring.
# 39 main columns, sixteen flattened LogUp columns on eleven buses, lqd 1; public values = the transcript root.
UINT256_PRECOMPILE_ID = 5689961814541250448     # `precompile_id("uint256")`: BLAKE3("miden-deferred-precompile/v1:7:uint256")[0..8] LE (core/src/deferred/precompile.rs:68-78)
CURVE_PRECOMPILE_ID = 7090426675861304240       # `precompile_id("curve")`; both checked against the library's BLAKE3 in tests/test_precompile_eval.py
TAG_AND_WORD = (1, 0, 0, 0)                                             # Tag::AND.as_word() (core/src/deferred/node.rs:53, :91-93)
UINT_PIN_CLAIM_TAG = 3                                                  # transcript/nodes.rs
VALUE_TAG_UINT, VALUE_TAG_GROUP = 1, 2                                  # transcript/binding.rs `ValueTag`
UINT_OP_IDS = dict(add=1, sub=2, mul=3, **{"is": 4})                    # UintPrecompile::{ADD,SUB,MUL,EQ}_OP_ID (precompiles/src/math/uint/precompile.rs:131-135)
EC_OP_IDS = dict(add=1, sub=2, **{"is": 3})                             # CurvePrecompile::{ADD,SUB,EQ}_OP_ID, MSM_OP_ID = 4 (curve/mod.rs:492-496)
EC_MSM_OP_ID = 4
TE_COLS, TE_AUX_COLS = 39, 16                                           # transcript/eval/mod.rs:110-306, :330-348
(TE_COL_ACT, TE_COL_PERM_SEQ_ID) = 0, 1
TE_COL_LHS, TE_COL_RHS, TE_COL_H = 2, 6, 10
(TE_COL_IS_ZERO, TE_COL_OUT_MULT, TE_COL_IS_AND, TE_COL_IS_UINT_LEAF, TE_COL_IS_UINT_OP, TE_COL_IS_EC_CREATE, TE_COL_IS_EC_PAI, TE_COL_IS_EC_OP,
 TE_COL_IS_ADD, TE_COL_IS_SUB, TE_COL_IS_MUL, TE_COL_IS_IS, TE_COL_IS_PINNED, TE_COL_PTR, TE_COL_BOUND_PTR, TE_COL_TAG_ARG1, TE_COL_A_PTR,
 TE_COL_B_PTR, TE_COL_TAG_ARG0, TE_COL_EC_GROUP_PTR, TE_COL_IS_EC_MSM, TE_COL_IS_MSM_LAST, TE_COL_MSM_IDX, TE_COL_MSM_EXPR, TE_COL_MSM_IS_HEAD) = range(14, 39)


def transcript_eval_air(host_aux=None):
    """`TranscriptEvalAir::eval` (transcript/eval/mod.rs:393-661) and its `LookupAir::eval` (:688-1164): col 0 consume-lhs (True) | 1
    consume-rhs + the True provide | 2, 3 the unhash permutation (rate0 + rate1 | capacity + digest) | 4 the leaf's UintVal | 5 the Uint /
    pinned provide | 6 the op children's Uint bindings | 7 UintAdd | 8 UintMul | 9 the EC operands' Group bindings | 10 the Group provide |
    11 EcPoint | 12 EcGroupAdd | 13 the MSM head's capacity | 14 the MSM term's child bindings | 15 MsmClaimTerm + MsmExpr."""
    b = dag.AirBuilder(TE_COLS, aux_width=TE_AUX_COLS, num_randomness=NUM_RANDOMNESS, num_aux_values=NUM_SIGMA_VALUES,
                       num_public=NUM_PUBLIC_VALUES)
    loc, nxt = [b.main(c) for c in range(TE_COLS)], [b.main(c, 1) for c in range(TE_COLS)]
    one, tr, first = b.const(1), b.is_transition(), b.is_first_row()
    act, is_zero, out_mult = loc[TE_COL_ACT], loc[TE_COL_IS_ZERO], loc[TE_COL_OUT_MULT]
    h = loc[TE_COL_H:TE_COL_H + 4]
    _assert_bool(b, act)
    b.assert_zero(tr * ((one - act) * nxt[TE_COL_ACT]))
    _assert_bool(b, is_zero)
    for h_i in h:
        b.assert_zero(is_zero * h_i)
    for i_ in range(4):
        b.assert_zero(first * (h[i_] - b.public(i_)))                   # the root pin: row 0's hash is the public transcript root
    b.assert_zero((one - act) * out_mult)
    is_and, is_uint_leaf, is_uint_op = loc[TE_COL_IS_AND], loc[TE_COL_IS_UINT_LEAF], loc[TE_COL_IS_UINT_OP]
    is_ec_create, is_ec_pai, is_ec_op = loc[TE_COL_IS_EC_CREATE], loc[TE_COL_IS_EC_PAI], loc[TE_COL_IS_EC_OP]
    is_ec_msm, is_msm_last, is_pinned = loc[TE_COL_IS_EC_MSM], loc[TE_COL_IS_MSM_LAST], loc[TE_COL_IS_PINNED]
    for col in (TE_COL_IS_AND, TE_COL_IS_UINT_LEAF, TE_COL_IS_UINT_OP, TE_COL_IS_EC_CREATE, TE_COL_IS_EC_PAI, TE_COL_IS_EC_OP, TE_COL_IS_EC_MSM,
                TE_COL_IS_MSM_LAST, TE_COL_IS_PINNED):
        _assert_bool(b, loc[col])
    b.assert_zero(is_msm_last * (one - is_ec_msm))
    is_add, is_sub, is_mul, is_is = loc[TE_COL_IS_ADD], loc[TE_COL_IS_SUB], loc[TE_COL_IS_MUL], loc[TE_COL_IS_IS]
    for col in (TE_COL_IS_ADD, TE_COL_IS_SUB, TE_COL_IS_MUL, TE_COL_IS_IS):
        _assert_bool(b, loc[col])
    is_op = is_add + is_sub + is_mul + is_is
    b.assert_zero(is_op - is_uint_op - is_ec_op)
    b.assert_zero(is_ec_op * is_mul)
    b.assert_zero(first * (is_zero + is_and + is_is + is_pinned - one))  # the root binds True
    is_create = is_ec_create + is_ec_pai
    for i_ in range(4):
        b.assert_zero(is_ec_pai * loc[TE_COL_LHS + i_])
        b.assert_zero(is_ec_pai * loc[TE_COL_RHS + i_])
    group_ptr = loc[TE_COL_EC_GROUP_PTR]
    is_result_op = is_op - is_is
    b.assert_zero(is_and + is_zero + is_uint_leaf + is_uint_op + is_ec_create + is_ec_pai + is_ec_op + is_ec_msm - act)
    not_uint_leaf = one - is_uint_leaf
    ptr, bound_ptr = loc[TE_COL_PTR], loc[TE_COL_BOUND_PTR]
    b.assert_zero(not_uint_leaf * is_pinned)
    b.assert_zero((not_uint_leaf - is_result_op - is_ec_create - is_ec_pai - is_msm_last) * ptr)
    b.assert_zero((not_uint_leaf - is_uint_op - is_ec_create - is_ec_msm) * bound_ptr)
    b.assert_zero((one - is_create) * (loc[TE_COL_TAG_ARG1] - (is_uint_leaf * bound_ptr + is_pinned * (ptr - bound_ptr))))
    a_ptr, b_ptr = loc[TE_COL_A_PTR], loc[TE_COL_B_PTR]
    b.assert_zero((one - is_op - is_ec_create - is_ec_msm) * a_ptr)
    b.assert_zero((one - is_op - is_ec_create - is_ec_msm) * b_ptr)
    b.assert_zero(is_is * (b_ptr - a_ptr))
    uint_op_id = is_add + is_sub * b.const(UINT_OP_IDS["sub"]) + is_mul * b.const(UINT_OP_IDS["mul"]) + is_is * b.const(UINT_OP_IDS["is"])
    ec_op_id = is_add * b.const(EC_OP_IDS["add"]) + is_sub * b.const(EC_OP_IDS["sub"]) + is_is * b.const(EC_OP_IDS["is"])
    b.assert_zero(loc[TE_COL_TAG_ARG0] - (is_pinned * bound_ptr + is_uint_op * uint_op_id + is_ec_op * ec_op_id))
    b.assert_zero((one - is_ec_op * (one - is_is) - is_ec_msm) * group_ptr)
    # the EcMsm absorb run: the head consumes the IV capacity, continuations run on the next Poseidon2 cycles, the tail reads the digest
    is_ec_msm_next, is_msm_head, is_msm_head_next = nxt[TE_COL_IS_EC_MSM], loc[TE_COL_MSM_IS_HEAD], nxt[TE_COL_MSM_IS_HEAD]
    _assert_bool(b, is_msm_head)
    b.assert_zero(is_msm_head * (one - is_ec_msm))
    continues = is_ec_msm * (one - is_msm_last)
    starts = is_ec_msm_next * (one - is_ec_msm + is_msm_last)
    b.assert_zero(first * (is_ec_msm * (is_msm_head - one)))
    b.assert_zero(tr * (continues * (one - is_ec_msm_next)))
    b.assert_zero(tr * (continues * is_msm_head_next))
    b.assert_zero(tr * (starts * (is_msm_head_next - one)))
    b.assert_zero(tr * (continues * (nxt[TE_COL_PERM_SEQ_ID] - loc[TE_COL_PERM_SEQ_ID] - one)))
    b.assert_zero(first * (is_ec_msm * loc[TE_COL_MSM_IDX]))
    b.assert_zero(tr * (starts * nxt[TE_COL_MSM_IDX]))
    b.assert_zero(tr * (continues * (nxt[TE_COL_MSM_IDX] - loc[TE_COL_MSM_IDX] - one)))
    b.assert_zero(tr * (continues * (nxt[TE_COL_MSM_EXPR] - loc[TE_COL_MSM_EXPR])))
    b.assert_zero(tr * (continues * (nxt[TE_COL_EC_GROUP_PTR] - loc[TE_COL_EC_GROUP_PTR])))

    lk = dag.LogUp(b, MAX_MESSAGE_WIDTH, NUM_BUS_IDS, closing="sigma_last_row")

    def message(bus, fields):            # fields: column numbers, ("const", v), or callables (bb, row) -> expression
        def msg(ch):
            bb = lk.b if ch is lk.ch_c else lk.lb
            row = [bb.main(c) for c in range(TE_COLS)]
            return ch.encode(bus, [row[f] if isinstance(f, int) else (bb.const(f[1]) if isinstance(f, tuple) else f(bb, row)) for f in fields])
        return msg
    K = lambda v: ("const", v)                                                            # noqa: E731
    cols = lambda at: [at + i_ for i_ in range(4)]                                        # noqa: E731

    def mults(fn):
        def both(bb):
            return fn(bb, [bb.main(c) for c in range(TE_COLS)])
        return both(lk.b), both(lk.lb)
    binding = lambda h_at, tag, ptr_f, bound_f: message(BUS_BINDING, cols(h_at) + [tag, ptr_f, bound_f])   # noqa: E731
    truth = lambda h_at: binding(h_at, K(VALUE_TAG_TRUE), K(0), K(0))                     # noqa: E731
    group_b = lambda h_at, ptr_col: binding(h_at, K(VALUE_TAG_GROUP), ptr_col, K(0))      # noqa: E731
    uint_b = lambda h_at, ptr_col: binding(h_at, K(VALUE_TAG_UINT), ptr_col, TE_COL_BOUND_PTR)   # noqa: E731
    p2_in = lambda tag, fields: message(BUS_POSEIDON2_IN, [TE_COL_PERM_SEQ_ID, K(tag)] + fields)   # noqa: E731
    f_create = lambda r: r[TE_COL_IS_EC_CREATE] + r[TE_COL_IS_EC_PAI]                     # noqa: E731
    f_node = lambda r: r[TE_COL_IS_AND] + r[TE_COL_IS_UINT_LEAF] + r[TE_COL_IS_UINT_OP] + f_create(r) + r[TE_COL_IS_EC_OP] + r[TE_COL_IS_EC_MSM]   # noqa: E731
    f_static = lambda r: r[TE_COL_IS_AND] + r[TE_COL_IS_UINT_LEAF] + r[TE_COL_IS_UINT_OP] + f_create(r) + r[TE_COL_IS_EC_OP]   # noqa: E731
    f_neg_out = lambda bb, r: bb.const(0) - r[TE_COL_OUT_MULT]                            # noqa: E731
    cap = [lambda bb, r: r[TE_COL_IS_AND] * bb.const(TAG_AND_WORD[0]) + (r[TE_COL_IS_UINT_LEAF] + r[TE_COL_IS_UINT_OP]) * bb.const(UINT256_PRECOMPILE_ID)
           + r[TE_COL_IS_PINNED] * (bb.const(UINT_PIN_CLAIM_TAG) - bb.const(UINT256_PRECOMPILE_ID)) + (f_create(r) + r[TE_COL_IS_EC_OP]) * bb.const(CURVE_PRECOMPILE_ID),
           lambda bb, r: r[TE_COL_IS_AND] * bb.const(TAG_AND_WORD[1]) + r[TE_COL_TAG_ARG0],
           lambda bb, r: r[TE_COL_IS_AND] * bb.const(TAG_AND_WORD[2]) + r[TE_COL_TAG_ARG1],
           lambda bb, r: r[TE_COL_IS_AND] * bb.const(TAG_AND_WORD[3])]
    transient = lambda bb, r: bb.const(1) - r[TE_COL_IS_PINNED]                           # noqa: E731
    add_or = lambda x_add, x_sub: (lambda bb, r: r[TE_COL_IS_ADD] * r[x_add] + r[TE_COL_IS_SUB] * r[x_sub])   # noqa: E731
    ec_result = lambda bb, r: r[TE_COL_IS_EC_OP] * (bb.const(1) - r[TE_COL_IS_IS])        # noqa: E731
    _emit_frac_cols(lk, [
        [(mults(lambda bb, r: r[TE_COL_IS_AND]), truth(TE_COL_LHS))],
        [(mults(lambda bb, r: r[TE_COL_IS_AND]), truth(TE_COL_RHS)),
         (mults(lambda bb, r: f_neg_out(bb, r) * (r[TE_COL_IS_AND] + r[TE_COL_IS_ZERO] + r[TE_COL_IS_IS])), truth(TE_COL_H))],
        [(mults(lambda bb, r: f_node(r)), p2_in(POSEIDON2_IN_TAG_RATE0, cols(TE_COL_LHS))), (mults(lambda bb, r: f_node(r)), p2_in(POSEIDON2_IN_TAG_RATE1, cols(TE_COL_RHS)))],
        [(mults(lambda bb, r: f_static(r)), p2_in(POSEIDON2_IN_TAG_CAP, cap)),
         (mults(lambda bb, r: f_node(r) - r[TE_COL_IS_EC_MSM] + r[TE_COL_IS_MSM_LAST]), message(BUS_POSEIDON2_OUT, [TE_COL_PERM_SEQ_ID] + cols(TE_COL_H)))],
        [(mults(lambda bb, r: r[TE_COL_IS_UINT_LEAF]), message(BUS_UINT_VAL, [TE_COL_PTR, TE_COL_BOUND_PTR] + cols(TE_COL_LHS) + cols(TE_COL_RHS)))],
        [(mults(lambda bb, r: f_neg_out(bb, r) * (r[TE_COL_IS_UINT_LEAF] + r[TE_COL_IS_UINT_OP] * (bb.const(1) - r[TE_COL_IS_IS]))),
          binding(TE_COL_H, lambda bb, r: transient(bb, r) * bb.const(VALUE_TAG_UINT), lambda bb, r: transient(bb, r) * r[TE_COL_PTR],
                  lambda bb, r: transient(bb, r) * r[TE_COL_BOUND_PTR]))],
        [(mults(lambda bb, r: r[TE_COL_IS_UINT_OP] + r[TE_COL_IS_EC_CREATE]), uint_b(TE_COL_LHS, TE_COL_A_PTR)),
         (mults(lambda bb, r: r[TE_COL_IS_UINT_OP] + r[TE_COL_IS_EC_CREATE]), uint_b(TE_COL_RHS, TE_COL_B_PTR))],
        [(mults(lambda bb, r: r[TE_COL_IS_UINT_OP] * (r[TE_COL_IS_ADD] + r[TE_COL_IS_SUB])),
          message(BUS_UINT_ADD, [TE_COL_BOUND_PTR, add_or(TE_COL_A_PTR, TE_COL_B_PTR), add_or(TE_COL_B_PTR, TE_COL_PTR), add_or(TE_COL_PTR, TE_COL_A_PTR), K(0)]))],
        [(mults(lambda bb, r: r[TE_COL_IS_MUL]),
          message(BUS_UINT_MUL, [K(1), K(0), TE_COL_A_PTR, TE_COL_B_PTR, TE_COL_BOUND_PTR, TE_COL_PTR, TE_COL_BOUND_PTR, K(0)]))],
        [(mults(lambda bb, r: r[TE_COL_IS_EC_OP]), group_b(TE_COL_LHS, TE_COL_A_PTR)), (mults(lambda bb, r: r[TE_COL_IS_EC_OP]), group_b(TE_COL_RHS, TE_COL_B_PTR))],
        [(mults(lambda bb, r: f_neg_out(bb, r) * (f_create(r) + ec_result(bb, r) + r[TE_COL_IS_MSM_LAST])), group_b(TE_COL_H, TE_COL_PTR))],
        [(mults(lambda bb, r: f_create(r)), message(BUS_EC_POINT, [TE_COL_PTR, TE_COL_TAG_ARG1, TE_COL_A_PTR, TE_COL_B_PTR, TE_COL_IS_EC_PAI]))],
        [(mults(ec_result), message(BUS_EC_GROUP_ADD, [TE_COL_EC_GROUP_PTR, add_or(TE_COL_A_PTR, TE_COL_PTR),
                                                       lambda bb, r: (r[TE_COL_IS_ADD] + r[TE_COL_IS_SUB]) * r[TE_COL_B_PTR], add_or(TE_COL_PTR, TE_COL_A_PTR)]))],
        [(mults(lambda bb, r: r[TE_COL_MSM_IS_HEAD]), p2_in(POSEIDON2_IN_TAG_CAP, [K(CURVE_PRECOMPILE_ID), K(EC_MSM_OP_ID), K(0), K(0)]))],
        [(mults(lambda bb, r: r[TE_COL_IS_EC_MSM]), group_b(TE_COL_LHS, TE_COL_A_PTR)), (mults(lambda bb, r: r[TE_COL_IS_EC_MSM]), uint_b(TE_COL_RHS, TE_COL_B_PTR))],
        [(mults(lambda bb, r: r[TE_COL_IS_EC_MSM]), message(BUS_MSM_CLAIM_TERM, [TE_COL_MSM_EXPR, TE_COL_A_PTR, TE_COL_B_PTR])),
         (mults(lambda bb, r: r[TE_COL_IS_MSM_LAST]),
          message(BUS_MSM_EXPR, [TE_COL_MSM_EXPR, TE_COL_EC_GROUP_PTR, TE_COL_PTR, lambda bb, r: r[TE_COL_MSM_IDX] + bb.const(1)]))]])
    lookup = lk.finish("transcript_eval")
    return dag.Air(b, _host_aux(lookup, host_aux), "transcript_eval"), lookup


K1_BOUND = 0xFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFEFFFFFC2E                                    # secp256k1: p - 1
K1_G = (0x79BE667EF9DCBBAC55A06295CE870B07029BFCDB2DCE28D959F2815B16F81798, 0x483ADA7726A3C4655DA4FBFC0E1108A8FD17B448A68554199C47D08FFB10D4B8)

