/*
 * mxpaillier — C ABI of the MI355X (gfx950) big-integer engine for the compute hot path of
 * TNO-MPC/protocols.distributed_keygen (distributed Paillier keygen + threshold decryption).
 *
 * The reference is pure Python; its arithmetic leaf is `pow_mod` / `mod_inv` of the un-vendored
 * package tno.mpc.encryption_schemes.utils (gmpy2 -> libgmp when installed), bound by name at
 *   src/tno/mpc/protocols/distributed_keygen/distributed_keygen.py:35   (DK)
 *   src/tno/mpc/protocols/distributed_keygen/paillier_shared_key.py:20  (PSK)
 * Each entry point below replaces one Python loop over those scalar calls; INTEGRATION.md shows
 * the ctypes binding a maintainer of the reference would add.
 *
 * Conventions
 *   - Big integers are little-endian arrays of `limbs` uint32 words ("rows"), element-major:
 *     element e occupies words [e*limbs, (e+1)*limbs).  This is `int.to_bytes(4*limbs,"little")`.
 *   - d_* pointers are DEVICE pointers (e.g. torch.Tensor.data_ptr()), h_* are HOST pointers.
 *   - The caller owns every buffer, including the workspace; the library allocates nothing that
 *     outlives a call (the one exception is explicit: mx_stream_create_cu_slice hands out a stream that
 *     the caller destroys), keeps no state between calls and reads no environment variable (the one exception is
 *     explicit too: mx_configure_hw_queues, the process set-up a caller opts into).  All work is enqueued on `stream` (a hipStream_t, NULL = default stream);
 *     calls return after enqueueing and NEVER synchronise the stream or the device.  Host arrays
 *     (h_*) travel by value in kernel-argument blocks and may be freed/reused on return; operand
 *     sets of thousands of moduli should use the *_dev entry points (device-resident operands).
 *   - Return value: MX_OK (0) or a negative MX_ERR_* code; nothing throws across the ABI.
 *   - Moduli must be odd and >= 3.  Supported modulus size: up to 16 700 bits.
 *   - Bases / partials must be < their modulus (the reference guarantees this: UT:361, PSK:92);
 *     values up to 16 * modulus (and < 2^(32*limbs)) are still reduced correctly.
 */
#ifndef MXPAILLIER_H
#define MXPAILLIER_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MX_OK 0
#define MX_ERR_ARG (-1)          /* null pointer / non-positive size */
#define MX_ERR_SIZE (-2)         /* modulus too large for the engine */
#define MX_ERR_MODULUS (-3)      /* even or < 3 modulus */
#define MX_ERR_WORKSPACE (-4)    /* workspace too small */
#define MX_ERR_HIP (-5)          /* a HIP runtime call failed (see mx_last_hip_error) */
#define MX_ERR_STATE (-6)        /* too late: the library has already used the GPU in this process */

/* ABI version (major*100 + minor). */
int mx_version(void);
const char* mx_error_string(int code);
/* hipGetErrorString of the last failing HIP call made by this library in this thread. */
const char* mx_last_hip_error(void);

/* ---- modular exponentiation ------------------------------------------------------------
 * Bytes of device workspace needed by mx_powmod_shared / mx_powmod_multi for these sizes. */
int64_t mx_powmod_workspace_bytes(int limbs, int exp_limbs, int64_t batch, int64_t groups);

/* d_out[e] = d_bases[e] ^ exp mod mod   for e in [0, batch): one modulus and one exponent for the
 * whole batch.  Replaces the loop `[secret_key.partial_decrypt(c) for c in ciphertext_sequence]`
 * (DK:463-466, single: DK:345-349) whose body is `pow_mod(c, exp, n_square)` (PSK:92), and any
 * other fixed-(exponent, modulus) batch (e.g. r^N mod N^2 of Paillier encryption).
 *   h_mod: limbs words, h_exp: exp_limbs words (exponent >= 0; a negative Lagrange exponent,
 *   PSK:89-91, is handled by the caller inverting the base, as the reference does). */
int mx_powmod_shared(const uint32_t* d_bases, uint32_t* d_out, const uint32_t* h_mod,
                     const uint32_t* h_exp, int limbs, int exp_limbs, int64_t batch,
                     void* d_workspace, int64_t workspace_bytes, void* stream);

/* d_out[g*group_size + k] = d_bases[g*group_size + k] ^ h_exps[g] mod h_mods[g].
 * Replaces the candidate loop DK:1313-1329 over __biprime_test_v_calculation, whose body is
 * `pow_mod(g, (N - p_i - q_i + 1) // 4, N)` (DK:1094) or `pow_mod(g, (p_i + q_i) // 4, N)`
 * (DK:1097): group g = candidate modulus, group_size = number of Jacobi-1 bases kept (40). */
int mx_powmod_multi(const uint32_t* d_bases, uint32_t* d_out, const uint32_t* h_mods,
                    const uint32_t* h_exps, int limbs, int exp_limbs, int64_t groups,
                    int64_t group_size, void* d_workspace, int64_t workspace_bytes, void* stream);

/* mx_powmod_shared with the lane geometry as an argument: limbs_per_lane 9 (narrow: more lanes per
 * element), 18 (wide: fewer, busier lanes), 3 (latency: many lanes per element, the exponentiation's products modulo
 * the friendly multiple of N — for launches that leave SIMDs idle, moduli up to 5533 bits), 6 (the bipartite latency form:
 * 3 limbs per lane, every product on two wavefronts, mx_powmod_launch_form) or 0 = automatic from an estimate of the
 * launch's duration: 6 while the launch leaves SIMDs idle, 3 up to about two such wavefronts per SIMD, else 9 or 18.
 * The same argument of mx_powmod_multi_dev and mx_powmod_geometry_for. */
int mx_powmod_shared_lpl(const uint32_t* d_bases, uint32_t* d_out, const uint32_t* h_mod, const uint32_t* h_exp,
                         int limbs, int exp_limbs, int64_t batch, int limbs_per_lane, void* d_workspace,
                         int64_t workspace_bytes, void* stream);

/* mx_powmod_multi with DEVICE-resident moduli and exponents (d_mods [groups][limbs], d_exps
 * [groups][exp_limbs]): the form for thousands of candidate moduli per keygen round (DK:1313-1329
 * with batch_size in the thousands) — nothing but launches is enqueued, and the moduli may be the
 * output of the device-side reconstruction of DK:1284.  mod_bits / exp_bits: upper bounds on the bit
 * lengths (they select the lane geometry and the number of exponent digits).  The moduli must be
 * odd and >= 3; this cannot be checked for device operands — an even modulus yields an unspecified
 * residue for its group, never a hang.  Workspace: mx_powmod_workspace_bytes. */
int mx_powmod_multi_dev(const uint32_t* d_bases, uint32_t* d_out, const uint32_t* d_mods, const uint32_t* d_exps,
                        int limbs, int exp_limbs, int mod_bits, int exp_bits, int64_t groups, int64_t group_size,
                        int limbs_per_lane, void* d_workspace, int64_t workspace_bytes, void* stream);

/* d_out[e] = d_bases[e] ^ exp mod N^2 with the modulus given by its ROOT h_n — the partial decryption
 * `pow_mod(ciphertext_value, exp, self.n_square)` of PSK:92 (n_square = n*n, PSK:46).  Same result
 * as mx_powmod_shared with the modulus N^2, computed with operations of the size of N only
 * (pairs x = rho*(X0 + X1*N), two half-size Montgomery passes per product; see mx_powmod_n2.hpp):
 * ~1.8x fewer multiply-accumulates and half the lanes per ciphertext.
 *   d_bases/d_out: [batch][limbs2] rows, limbs2 >= words of N^2;  h_n: limbs_n words;  h_exp: exp_limbs
 *   words (exponent >= 0); bases must be < N^2. */
int64_t mx_powmod_nsquare_workspace_bytes(int limbs_n, int exp_limbs, int64_t batch);
int mx_powmod_nsquare(const uint32_t* d_bases, uint32_t* d_out, const uint32_t* h_n, const uint32_t* h_exp,
                      int limbs_n, int limbs2, int exp_limbs, int64_t batch, void* d_workspace,
                      int64_t workspace_bytes, void* stream);

/* ---- per-key plans ------------------------------------------------------------------------
 * Everything mx_powmod_nsquare derives from (N, exp) — the N-adic constant pairs, C', and the tape
 * (conversion, table of odd powers, sliding-window schedule) — depends on the KEY only: N is the
 * public modulus (PSK:46) and exp the party's Lagrange-folded share (PSK:79-85), both fixed for the
 * life of a PaillierSharedKey.  prepare derives them once (about 1 ms of host work) and writes them
 * into a caller-owned device block; run launches the modexp kernel and nothing else: no host
 * arithmetic, no operand upload.  The plan descriptor is a plain struct the caller keeps on the
 * host; the device block must stay valid, and the stream passed to prepare must be complete or
 * ordered before the streams passed to run (prepare's uploads are enqueued on it).
 * limbs_per_lane of run: 9 (narrow geometry), 18 (wide), 3 (latency geometry, two wavefronts per group only)
 * or 0 = the library's choice.
 * wavefronts_per_group of run: 1 = one wavefront executes both Montgomery passes of every pair product; 2 = the
 * passes run on two wavefronts of one workgroup, the second one operation behind the first (the chain of first
 * N-adic digits never reads the second digits) — 0.54-0.58 of the time per operation with twice the wavefronts,
 * for launches that leave SIMDs idle: a single ciphertext (PSK:92 called from DK:345-349), a keygen-sized batch,
 * one 10 000-ciphertext sequence; 4 (ABI 4.3; limbs_per_lane 3 or 0; moduli whose groups have 16, 32 or 64 lanes: key_length
 * 1024, 2048 and 4096 — ~800 .. 2560 and ~2800 .. 5500 bits, MX_ERR_SIZE elsewhere) = BOTH passes bipartite on two wavefronts each — four wavefronts per group of elements and a fifth that
 * forms the quotient correction one product behind —, the shortest dependent chain there is, for launches of at most one
 * workgroup per compute unit (a lone decrypt: 9.4 instead of 12.95 ms at key_length 2048, 31.8 instead of 47 at 4096); 0 = the library's choice (which takes 4 for such launches).  With both at 0 the library estimates the duration
 * of ONE launch of this batch on an idle GPU for every shape and takes the shortest; callers that keep several
 * launches in flight fill the machine between them and should pass 18 / 1.  mx_nsquare_launch_shape reports the
 * choice.  Same result bit for bit in every shape.
 * segments of run: the exponentiation is enqueued as this many consecutive launches, each executing a
 * stretch of the tape (the accumulator travels through the workspace); a wavefront then lives
 * 1/segments as long, which is the grain at which a burst of launches on several streams drains.
 * 1..64, 0 = automatic (4 for long exponents on large batches, else 1).  Same result bit for bit.
 * A two-wavefront launch with somewhat more groups of elements than the GPU holds at once runs in the time-sliced
 * form (mx_nsquare_launch_timesliced): ONE launch of resident workgroups whose wavefront pairs take the segments of
 * all groups from queues kept in the workspace (the group with the most work left first); `segments` (at most 16 then)
 * is the number of units per group. */
typedef struct mx_nsquare_plan {
  const void* d_plan;     /* device block written by prepare */
  int64_t plan_bytes;
  int32_t limbs_n;        /* words of N */
  int32_t n_bits;
  int32_t exp_bits;
  int32_t window;         /* sliding-window width of the tape (table of 2^(window-1) odd powers) */
  int32_t ntape;          /* tape words */
  int32_t n_sqr;          /* pair squarings one exponentiation executes */
  int32_t n_mul;          /* pair multiplications one exponentiation executes */
  int32_t geometries;     /* bits 0-7: mask of the limbs_per_lane values with a kernel instance for this modulus: 1 = 9, 2 = 18,
                           * 4 = 3; 8 = the plan holds the constants of the five-wavefront latency form.  Bits 8-15: the pivot
                           * (multiplier limbs on the L wavefronts, at most 192) those constants were built with;
                           * mx_powmod_nsquare_run takes the form's pivot from here, not from MX_KNOB_BI_PIVOT, and refuses a
                           * value that does not fit the geometry with MX_ERR_ARG.  0 there (a plan written by a library
                           * before this field carried it): the pivot of the knob at the time of the run. */
  int32_t n_slot_reads;   /* pair slots (2 * limbs_per_lane words per lane) one exponentiation reads from ... */
  int32_t n_slot_writes;  /* ... and writes to the workspace: the kernel's HBM traffic model */
  /* The lifted tape.  For a = b (mod N), a^N = b^N (mod N^2); so with exp = e1 N + e0, 0 <= e0 < N,
   *     x^exp = (x^e1 mod N)^N * x^e0   (mod N^2):
   * x^e1 modulo N is the chain of FIRST digits of the pair arithmetic — pass 1 of a squaring or multiplication, no pass
   * 2 — and y^N x^e0 is one two-base sliding-window exponentiation whose bits(N) squarings both bases share.  For the
   * 4197-bit share exponent of key_length 2048 that is ~2145 first-digit and ~2050 pair squarings instead of 4196 pair
   * squarings: ~0.81 of the instructions by the planner's model.  prepare builds this tape NEXT TO the classic one whenever
   * exp >= N (never for MX_PLAN_FIXED_WINDOW plans, whose point is a sequence that depends on the exponent's length
   * only, and never for exp < N, which covers every encryption-type exponent) and marks it as preferred where its
   * estimated cost is lower; mx_powmod_nsquare_run takes it for one-wavefront launches (wavefronts_per_group 1) as
   * MX_KNOB_N2_LIFT says.  The two-wavefront, time-sliced and five-wavefront forms always read the classic tape.
   * n_sqr, n_mul, n_slot_reads and n_slot_writes above describe the tape a one-wavefront launch runs by default: the
   * lifted one where `lift` has bit 1 set (n_sqr and n_mul then count its PAIR operations only), else the classic one.
   * Same results bit for bit either way.  A descriptor with these fields zero is a plan without a lifted tape. */
  int32_t n_sqr_first;    /* first-digit squarings of that tape (0: the classic tape) */
  int32_t n_mul_first;    /* first-digit multiplications of that tape */
  int32_t table_rows;     /* pair slots of the table region (from slot 8 on) that the largest of the plan's tapes needs */
  int32_t lift;           /* bit 0: the plan holds a lifted tape; bit 1: the planner's cost model prefers it */
  int32_t ntape_lift;     /* words of the lifted tape */
  int32_t n_sqr_classic;  /* pair squarings and ... */
  int32_t n_mul_classic;  /* ... multiplications of the classic tape, whichever is the default */
  int32_t lift_positions; /* lifted tape: squarings of either kind (tape positions), ... */
  int32_t lift_pos1;      /* ... those in front of its second phase, and ... */
  int32_t lift_share1;    /* ... their share of the tape's estimated cost, in 1/65536: run cuts segments by cost */
} mx_nsquare_plan;
int64_t mx_nsquare_plan_bytes(int limbs_n, int exp_limbs);
/* Host only (no device, no stream): the tape prepare_ex would write for (N, exp, flags) — lifted = 0 the classic tape,
 * 1 the lifted one — into h_tape[0 .. max_words), and the descriptor's counting fields into *plan (d_plan = NULL).
 * Word = (op << 28) | argument; ops 0 SQR k, 1 MUL slot, 2 ADD slot, 3 LOAD slot, 4 STORE slot, 5 MULC slot (the last
 * product), 6 SQR0 k, 7 MUL0 slot (first-digit forms), 8 CLR1 (second digit := 0); slots 0-7 constants and scratch,
 * 8.. table rows.  Returns the number of words (0: no such tape for this plan), MX_ERR_WORKSPACE if max_words is too
 * small, or the error prepare_ex would return.  For checking the schedule on a machine without a GPU. */
int mx_nsquare_tape(const uint32_t* h_n, const uint32_t* h_exp, int limbs_n, int exp_limbs, int flags, int lifted,
                    uint32_t* h_tape, int max_words, mx_nsquare_plan* plan);
int mx_powmod_nsquare_prepare(mx_nsquare_plan* plan, const uint32_t* h_n, const uint32_t* h_exp, int limbs_n,
                              int exp_limbs, void* d_plan, int64_t plan_bytes, void* stream);
/* The same with options (flags = 0: exactly mx_powmod_nsquare_prepare).
 * MX_PLAN_FIXED_WINDOW: a fixed-window tape — w squarings and ONE multiplication per w-bit window, a window of zero
 * bits multiplying by the domain's one — instead of the sliding-window tape, whose runs of squarings and number of
 * multiplications are a function of the exponent's bits.  The exponent is the party's Lagrange-folded secret share
 * (PSK:79-85): with this flag the sequence and number of operations a launch executes, hence its duration and the
 * kernel-trace of a profiler, depend on the exponent's LENGTH only.  The table row a window reads is still selected by
 * the secret digit (addresses, not timing of the instruction stream).  Cost: 728 instead of 592 pair multiplications
 * for a 4197-bit exponent (w = 7: a 127-row table instead of 64 odd powers, twice the workspace) = +3.6 % instructions.  plan->window then reports w + 1 (the
 * table region is sized as 2^(window - 1) rows either way).  Same results bit for bit.  A fixed-window plan holds no
 * lifted tape (mx_nsquare_plan): the split of the exponent at N and the merged windows of its second phase would make
 * the sequence of operations depend on more than the exponent's length. */
#define MX_PLAN_FIXED_WINDOW 1
int mx_powmod_nsquare_prepare_ex(mx_nsquare_plan* plan, const uint32_t* h_n, const uint32_t* h_exp, int limbs_n,
                                 int exp_limbs, int flags, void* d_plan, int64_t plan_bytes, void* stream);
/* workspace of one run (the table of odd powers of every base; one per launch in flight) */
int64_t mx_powmod_nsquare_run_workspace_bytes(const mx_nsquare_plan* plan, int64_t batch);
int mx_powmod_nsquare_run(const mx_nsquare_plan* plan, const uint32_t* d_bases, uint32_t* d_out, int limbs2,
                          int64_t batch, int limbs_per_lane, int wavefronts_per_group, int segments,
                          void* d_workspace, int64_t workspace_bytes, void* stream);

/* ---- small-prime sieve -----------------------------------------------------------------
 * d_out[e] = 1 if some h_primes[k] divides candidate e else 0.  Replaces
 * `__small_prime_divisors_test(prime_list, n)` (DK:1197-1209) looped over the batch of
 * candidates at DK:1288-1292.  Primes must be odd, >= 3 and < 2^31; limbs <= 1024
 * (lists whose largest prime is below 2^21 — the reference's default threshold is 2000 — run without any
 * intermediate reduction; larger ones fold the 64-bit columns every floor(2^32 / max prime) - 1 limbs). */
int64_t mx_sieve_workspace_bytes(int limbs, int n_primes);
int mx_sieve(const uint32_t* d_candidates, uint8_t* d_out, const uint32_t* h_primes, int n_primes,
             int limbs, int64_t batch, void* d_workspace, int64_t workspace_bytes, void* stream);

/* ---- share recombination ---------------------------------------------------------------
 * For every ciphertext e:  x = prod_{i<n_partials} d_partials[i][e] mod N^2;
 *   d_status[e] = 1 and d_out[e] = 0           if (x - 1) % N != 0   (PSK:119-123 -> ValueError)
 *   d_status[e] = 0 and d_out[e] = ((x - 1) / N * theta_inv) % N     (PSK:125)
 * Replaces `PaillierSharedKey.decrypt` (PSK:95-127) looped at DK:510-515 (single: DK:378-380).
 *   d_partials: [n_partials][batch][limbs2] words, residues mod N^2 (players 1..degree+1 in order)
 *   h_n: limbs words (N; N^2 is derived), h_theta_inv: limbs words; limbs2 >= words of N^2
 *   d_out: [batch][limbs] words. */
int64_t mx_combine_workspace_bytes(int limbs, int limbs2, int n_partials, int64_t batch);
int mx_combine(const uint32_t* d_partials, uint32_t* d_out, uint8_t* d_status, const uint32_t* h_n,
               const uint32_t* h_theta_inv, int limbs, int limbs2, int n_partials, int64_t batch,
               void* d_workspace, int64_t workspace_bytes, void* stream);

/* Per-key plan of the recombination (N, N^2, the Montgomery constants and theta_inv depend on the
 * key only, PSK:46-50): prepare once, then run enqueues the kernel and nothing else.  Rows of d_out
 * are out_stride >= limbs words wide; if out_stride > limbs, word [limbs] of every row receives the
 * status (0 / 1) and the remaining words are zero, so that plaintext and status travel as ONE row
 * (one all-gather when ciphertexts are sharded over GPUs); d_status may then be NULL. */
typedef struct mx_combine_plan {
  const void* d_plan;
  int64_t plan_bytes;
  int32_t limbs, limbs2, n_bits, n2_bits;
} mx_combine_plan;
int64_t mx_combine_plan_bytes(int limbs, int limbs2);
int mx_combine_prepare(mx_combine_plan* plan, const uint32_t* h_n, const uint32_t* h_theta_inv, int limbs,
                       int limbs2, void* d_plan, int64_t plan_bytes, void* stream);
int mx_combine_run(const mx_combine_plan* plan, const uint32_t* d_partials, uint32_t* d_out, int out_stride,
                   uint8_t* d_status, int n_partials, int64_t batch, void* stream);
/* The plan's constant rows as the host builds them, without a device: 3 + MX_COMBINE_NP_MAX rows of limbs2 words, zero
 * padded — N | N^2 | theta_inv * R1 mod N | R2^k mod N^2 for k = 1 .. MX_COMBINE_NP_MAX — with R1 = 2^(w l b1) and
 * R2 = 2^(w l b2) the Montgomery radices of N and N^2 in the lane geometry of N^2 (mx_geometry of bits(N^2): lanes,
 * l, w, b2; b1 = ceil((bits(N) + 4) / (w l))).  A run with n_partials <= MX_COMBINE_NP_MAX multiplies the raw rows
 * and then by R2^n_partials: n_partials products modulo N^2; with more partials it converts every row (2 n_partials).
 *   MX_ERR_WORKSPACE if rows_words is less than that many words; the other errors are those of the prepare call. */
#define MX_COMBINE_NP_MAX 8
int mx_combine_constants(const uint32_t* h_n, const uint32_t* h_theta_inv, int limbs, int limbs2, uint32_t* h_rows,
                         int64_t rows_words);

/* ---- biprimality verdict ---------------------------------------------------------------
 * d_pass[g*n_slots + k] = 1 iff  v_1 == +-prod_{i>=2} v_i (mod N_g) for test slot k, where
 * d_v is [n_parties][groups][n_slots][limbs] (party index 1 first).  Replaces the per-slot test
 * of __biprime_test_with_v_i (DK:1147-1158); the caller ANDs the slots (DK:1160-1172). */
int64_t mx_verdict_workspace_bytes(int limbs, int n_parties, int64_t groups, int64_t n_slots);
int mx_biprime_verdict(const uint32_t* d_v, uint8_t* d_pass, const uint32_t* h_mods, int limbs,
                       int n_parties, int64_t groups, int64_t n_slots, void* d_workspace,
                       int64_t workspace_bytes, void* stream);

/* The same with device-resident moduli (d_mods [groups][limbs], all odd and >= 3, at most mod_bits
 * bits); workspace: mx_verdict_workspace_bytes. */
int mx_biprime_verdict_dev(const uint32_t* d_v, uint8_t* d_pass, const uint32_t* d_mods, int limbs, int mod_bits,
                           int n_parties, int64_t groups, int64_t n_slots, void* d_workspace,
                           int64_t workspace_bytes, void* stream);

/* ---- modular multiplication ------------------------------------------------------------
 * d_out[e] = d_a[e] * d_b[e] mod h_mod.  The glue around the modexps: (1 + mN) * r^N of Paillier
 * encryption (the un-vendored tno.mpc.encryption_schemes.paillier used by the reference's tests,
 * test_distributed_keygen.py:125), homomorphic addition, and the product tree of the batched
 * modular inversion that replaces `mod_inv(ciphertext_value, n_square)` per ciphertext (PSK:89-91).
 * d_out may alias d_a or d_b. */
int64_t mx_mulmod_workspace_bytes(int limbs);
int mx_mulmod_shared(const uint32_t* d_a, const uint32_t* d_b, uint32_t* d_out, const uint32_t* h_mod,
                     int limbs, int64_t batch, void* d_workspace, int64_t workspace_bytes, void* stream);

/* ---- Shamir-field arithmetic of the candidate moduli ---------------------------------------
 * The key generation holds p, q and a sharing of zero as Shamir shares modulo a prime P of
 * 2*(prime_length + log2(parties)) bits (DK:647-651).  Per candidate of a round:
 *   mx_fma_mod      d_out[e] = (d_a[e] * d_b[e] + d_c[e]) mod P — this party's share of N,
 *                   `prime_candidate_p * prime_candidate_q` then `candidate_n += zero` (DK:1274-1277;
 *                   ShamirVariable.__mul__ / __add__, UT:205-250)
 *   mx_lincomb_mod  d_out[e] = sum_t h_coeffs[t] * d_x[t][e] mod P — `candidate_n.reconstruct()`
 *                   (DK:1284; UT:263-270, 465-471) with the Lagrange coefficients at 0 of the
 *                   parties' evaluation points; d_x is [terms][batch][limbs], h_coeffs [terms][limbs].
 * P odd; operands < P (values up to 16 P are still reduced correctly).  The reconstructed moduli
 * are exactly the rows mx_sieve / mx_jacobi_dev / mx_powmod_multi_dev take. */
int64_t mx_field_workspace_bytes(int limbs, int terms);
int mx_fma_mod(const uint32_t* d_a, const uint32_t* d_b, const uint32_t* d_c, uint32_t* d_out, const uint32_t* h_mod,
               int limbs, int64_t batch, void* d_workspace, int64_t workspace_bytes, void* stream);
int mx_lincomb_mod(const uint32_t* d_x, const uint32_t* h_coeffs, uint32_t* d_out, const uint32_t* h_mod, int limbs,
                   int terms, int64_t batch, void* d_workspace, int64_t workspace_bytes, void* stream);

/* ---- modular inverse ------------------------------------------------------------------------
 * d_out[e] = d_values[e]^-1 mod h_mod, d_status[e] = 0; or d_out[e] = 0, d_status[e] = 1 when
 * gcd(value, modulus) != 1 (where `pow(v, -1, m)` raises ValueError).  Replaces `mod_inv(theta, n)`
 * of a key (PSK:50) and — as the root of a product tree of mx_mulmod_shared launches (Montgomery's
 * trick: 3 multiplications per element) — `mod_inv(ciphertext_value, n_square)` per ciphertext for
 * a negative Lagrange exponent (PSK:89-91).  One wavefront per element (the big integers are spread
 * over its 64 lanes): meant for a handful of elements, ~1-4 ms each at 2048-8200 bits. */
int64_t mx_modinv_workspace_bytes(int limbs);
int mx_modinv(const uint32_t* d_values, uint32_t* d_out, uint8_t* d_status, const uint32_t* h_mod, int limbs,
              int64_t batch, void* d_workspace, int64_t workspace_bytes, void* stream);

/* ---- Jacobi symbol ---------------------------------------------------------------------
 * d_out[g*group_size + k] = Jacobi symbol (d_values[g*group_size + k] / h_mods[g]) in {-1, 0, +1}.
 * Replaces the filter `sympy.jacobi_symbol(g, modulus) != 1` of the biprimality test (DK:1089),
 * evaluated for the up to 4*40 jointly random generators of every candidate (DK:1028, 1084-1099).
 * Values must be < their modulus (UT:361); moduli odd; limbs <= 257 (8224 bits: key_length 8192,
 * the widest key whose N^2 the modexp kernels take). */
int64_t mx_jacobi_workspace_bytes(int limbs, int64_t groups);
int mx_jacobi(const uint32_t* d_values, int8_t* d_out, const uint32_t* h_mods, int limbs, int64_t groups,
              int64_t group_size, void* d_workspace, int64_t workspace_bytes, void* stream);

/* The same with device-resident moduli (no workspace). */
int mx_jacobi_dev(const uint32_t* d_values, int8_t* d_out, const uint32_t* d_mods, int limbs, int64_t groups,
                  int64_t group_size, void* stream);
/* Only the rows [first, first + count) of every group (d_out entries outside the range are left
 * untouched); with d_skip_counts given, groups whose d_skip_counts[g] >= skip_threshold are not
 * evaluated at all.  The v-calculation stops at correct_param_biprime generators with symbol 1
 * (DK:1086): the head of the generator list almost always yields them, so the tail is evaluated
 * only for the candidates where it did not — the same selection as the reference, ~35 % fewer symbols. */
int mx_jacobi_dev_range(const uint32_t* d_values, int8_t* d_out, const uint32_t* d_mods, int limbs, int64_t groups,
                        int64_t group_size, int first, int count, const int32_t* d_skip_counts, int skip_threshold,
                        void* stream);

/* ---- selection of the generators -------------------------------------------------------
 * For every group, copies the first `keep` rows whose flag is 1 (in order) to d_out[g][0..keep) and
 * stores how many were found in d_counts[g]; unfilled rows are zero.  With d_flags = the output of
 * mx_jacobi this is `if jacobi_symbol(g, N) != 1: continue` + `stop at correct_param_biprime` of
 * the v-calculation loop (DK:1084-1099), so the generators never leave the device between the
 * Jacobi filter and mx_powmod_multi. */
int mx_select_first(const uint32_t* d_rows, const int8_t* d_flags, uint32_t* d_out, int32_t* d_counts,
                    int limbs, int64_t groups, int group_size, int keep, void* stream);

/* ---- diagnostics -----------------------------------------------------------------------
 * Runs the DPP cross-lane primitives against their ds_bpermute reference forms for every group
 * width on the current device; returns the number of mismatching lanes (0 = pass) or MX_ERR_*. */
int mx_selftest_lanes(void* stream);
/* Developer overrides, explicit calls only (the library reads no environment variables).  value 0 restores
 * the default.  MX_KNOB_N2_SEGMENTS: launches per mx_powmod_nsquare_run exponentiation when the caller passes
 * segments = 0 (1..64).  MX_KNOB_JACOBI_MAX_BATCHES: value v > 0 limits the Jacobi kernel to v - 1 divstep batches
 * so that its fallback kernel has to finish the symbols (test knob for the safety net).  MX_KNOB_N2_TIMESLICE: the
 * time-sliced form of two-wavefront launches (resident workgroups that share the groups of elements segment by
 * segment): 0 = where the estimate favours it, 1 = never, 2 = always, 16 + r = always, with r
 * workgroups per CU (r = 1..3).  MX_KNOB_N2_FRIENDLY_1W: 1 = the one-wavefront wide kernel never takes its
 * friendly-modulus instances (A/B runs against the plain ones).  MX_KNOB_GENERIC_LATENCY: 1 = the automatic geometry of
 * the generic-modulus modexp never takes the 3-limb latency instances (one or two wavefronts), 2 = never the bipartite form.  MX_KNOB_N2_SPLIT: mx_nsquare_launch_split
 * 1 = never reports a split, 2 = whenever one exists.  These are the ONLY process-wide settings the library has (ABI 4.0
 * dropped mx_set_limbs_per_lane: launch shapes are call arguments, the entry points without one leave the choice to the
 * library); each is an atomic integer, so flipping one while another thread launches is well defined (that launch sees
 * the old or the new value).  Production callers never need them.  Returns MX_OK / MX_ERR_ARG. */
#define MX_KNOB_N2_SEGMENTS 1
#define MX_KNOB_JACOBI_MAX_BATCHES 2
#define MX_KNOB_N2_TIMESLICE 3
#define MX_KNOB_N2_FRIENDLY_1W 4
#define MX_KNOB_GENERIC_LATENCY 5
#define MX_KNOB_N2_SPLIT 6
#define MX_KNOB_LAT_LANES 8         /* 3-limb latency forms of the generic kernel: at least this many lanes per element (0 = the smallest group that holds the number) */
#define MX_KNOB_N2_BIPAIR 9         /* 1 = mx_powmod_nsquare_run never chooses the five-wavefront latency form by itself (A/B runs) */
#define MX_KNOB_BI_PIVOT 7          /* bipartite form of the generic kernel: multiplier limbs on the Montgomery wavefront (0 = the library's pivot) */
#define MX_KNOB_N2_LIFT 10          /* the lifted tape of mx_powmod_nsquare_run's one-wavefront launches (mx_nsquare_plan): 0 = never, 1 = whenever the plan
                                     * holds one, 2 = where the planner's cost model prefers it — the default, so for THIS knob 2, not 0, restores it.  Read
                                     * by run, not by prepare: a plan prepared under one value runs correctly under any other */
int mx_debug_knob(int knob, int value);
/* Enqueues a kernel of ONE wavefront that idles for `microseconds` (0..1 000 000) on `stream` and touches no
 * memory.  A concurrency probe: two streams that the HIP runtime has mapped to the same hardware queue run
 * their spins one after the other, two streams on different queues run them side by side — which is what
 * decides whether chunks of a batch launched on those streams fill the machine together or serialise
 * (GPU_MAX_HW_QUEUES is read once when the runtime initialises and cannot be queried: mx_configure_hw_queues sets it
 * in time, mx_stream_census below is this probe run over a set of streams).  Never synchronises. */
int mx_spin(int64_t microseconds, void* stream);
/* Process set-up for callers that keep several launches in flight on streams of their own: the HIP runtime maps the
 * streams of a process onto GPU_MAX_HW_QUEUES hardware queues — 4 when the variable is unset, and job runners commonly
 * export 4 as well —, two streams on one queue serialise their kernels, and four launches of this library that were
 * meant to fill the machine together then run 2.3 at a time (profiles/r27_overlap_before.txt).  Call it BEFORE the
 * first GPU call of the process (of anybody: the runtime reads the variable once, when it initialises).  Makes no HIP
 * call.  `queues` is clamped to 1..32 and written to GPU_MAX_HW_QUEUES (setenv, process-wide, inherited by child
 * processes) when the variable is unset, is not a positive number, or is SMALLER than the request: an inherited
 * value does not silently undercut what the caller asked for; a larger inherited value stays.  The library never
 * writes a value above 32.  MX_HW_QUEUES_KEEP=1 in the environment is the opt-out of a user who really wants fewer
 * queues: nothing is changed.  Returns the value the environment holds afterwards (0: unset — the runtime's default),
 * or MX_ERR_STATE without changing anything if this library has already made a GPU call in the process (it cannot
 * see the GPU calls of others: a caller that initialised the runtime by other means gets the value back, and the
 * census tells what it really got). */
int mx_configure_hw_queues(int queues);
/* What mx_configure_hw_queues last wrote or found in this process; 0 if it was never called (or found nothing and
 * was told to keep that). */
int mx_hw_queues_configured(void);
/* Which of the caller's `n` (1..64) streams run side by side, measured with mx_spin: stream 0 is accepted and sets
 * the time of one spin of `spin_us` microseconds (1..1 000 000; best of four rounds); every further stream spins
 * together with the streams accepted so far and is accepted if the set still takes less than 1.6 spins.  group_of[i]
 * = i for an accepted stream; for a stream that was not accepted the index of the first accepted stream it
 * serialises with when the two spin alone, or -1 if it runs beside each of them alone and only the whole set was
 * slower (a limit on the set, not a shared queue — the one case in which no accepted stream can be named).  Naming
 * the partner costs every stream that is NOT accepted ceil(log2(accepted)) + 1 further probes of two rounds each (the
 * accepted streams are halved until one is left); accepted streams cost nothing extra.  Returns the number of accepted
 * streams or MX_ERR_ARG / MX_ERR_HIP.  Unlike every
 * other entry point it WAITS: for the device first, then for the given streams after every round — a set-up call,
 * not one for the hot path. */
int mx_stream_census(void* const* streams, int n, int64_t spin_us, int* group_of);
/* Streams confined to a slice of the compute units, for callers that keep several SMALL launches in flight: the
 * dispatcher places concurrent launches of a few dozen workgroups each on the same CUs of every XCD (four 64-workgroup
 * launches on four ordinary streams ran 1.7x longer than one of them alone), while launches on streams whose CU
 * masks are disjoint each get their own part of the chip.  Slice k of n is the same CU range [k*CUs/n, (k+1)*CUs/n) of
 * the mask in EVERY XCD (mask bit i = CU i/8 of XCD i%8 on MI355X; a mask that empties an XCD is ignored by the
 * runtime), n <= 8.  The stream belongs to the caller (mx_stream_destroy).  Not for launches that fill the machine
 * on their own: a static partition cannot balance load. */
int mx_stream_create_cu_slice(int slice, int n_slices, int reserved, void** stream_out);
int mx_stream_destroy(void* stream);
/* Enqueues a kernel of ONE wavefront that idles for `microseconds` and writes two counters to d_ticks[0..1]: the
 * advance of the shader clock counter and of the 100 MHz real-time counter over that interval; their ratio x 100 MHz
 * is the clock the SIMDs run at under the load that is in flight at that moment (MI355X drops from its nominal
 * 2.4 GHz to ~2.1 GHz when every SIMD streams multiply-accumulates: profiles/r03_ubench_valu_peak.txt).  Launch it
 * on a stream of its own while the work of interest runs.  Never synchronises. */
int mx_clock_probe(int64_t microseconds, uint64_t* d_ticks, void* stream);
/* Engine geometry chosen for a modulus of `mod_bits` bits: lanes per element (K), limbs per lane
 * (L), limb width (W) and Montgomery blocks; returns MX_OK or MX_ERR_SIZE. */
int mx_geometry(int mod_bits, int* lanes_per_element, int* limbs_per_lane, int* limb_bits, int* blocks);
/* Kernel timing for benchmarks.  mx_profile(1): every following mx_powmod_shared / mx_powmod_multi /
 * mx_powmod_nsquare call records two events on its stream around its modexp kernel (after the operand
 * uploads; mx_powmod_nsquare_run and mx_powmod_multi_dev are timed too).  mx_profile_collect waits for all recorded launches and returns the sum of their durations
 * and their number, then forgets them.  mx_profile(0) stops recording.  Returns MX_OK / MX_ERR_HIP. */
int mx_profile(int enable);
int mx_profile_collect(double* total_ms, int* launches);
/* Geometry mx_powmod_nsquare launches for a modulus N of `n_bits` bits and `batch` bases (it depends
 * on the batch: the wide geometry is chosen when one launch brings enough wavefronts); returns MX_OK or
 * MX_ERR_SIZE. */
int mx_nsquare_geometry(int n_bits, int64_t batch, int* lanes_per_element, int* limbs_per_lane, int* limb_bits,
                        int* blocks);

/* Geometry for an explicit limbs_per_lane (9 | 18 | 0 = the library's automatic choice for this
 * batch): of a mx_powmod_nsquare_run launch, and of a
 * mx_powmod_shared_lpl (groups = 1) / mx_powmod_multi_dev (groups > 1) launch. */
int mx_nsquare_geometry_for(int n_bits, int64_t batch, int limbs_per_lane, int* lanes_per_element,
                            int* limbs_per_lane_out, int* limb_bits, int* blocks);
/* The full launch shape mx_powmod_nsquare_run uses for (limbs_per_lane, wavefronts_per_group), either or both 0 =
 * the library's choice for this batch: the geometry as above plus the wavefronts per group of elements (1 | 2). */
int mx_nsquare_launch_shape(int n_bits, int64_t batch, int limbs_per_lane, int wavefronts_per_group,
                            int* lanes_per_element, int* limbs_per_lane_out, int* limb_bits, int* blocks,
                            int* wavefronts_per_group_out);
/* For callers that keep SEVERAL launches in flight which together process `total` elements (several streams, several
 * keys): the shape to pass to each of them — the plain form with the lowest estimate for one launch of the total, never a
 * time-sliced one (only a lone launch can be that).  Arguments as mx_nsquare_launch_shape; ABI 4.2. */
int mx_nsquare_pieces_shape(int n_bits, int64_t total, int limbs_per_lane, int wavefronts_per_group,
                            int* limbs_per_lane_out, int* wavefronts_per_group_out);
/* Whether mx_powmod_nsquare_run runs this launch in the time-sliced form of the two-wavefront kernel: a fixed number
 * of resident workgroups per CU that take (segment, group of elements) units from a queue in the workspace, chosen
 * when a lone launch has somewhat more groups than the GPU holds at once (e.g. 10 000 ciphertexts at key_length
 * 2048: 41 ms instead of 52-60; 18 limbs per lane, one workgroup per CU, 8 units per group).  *resident_per_cu = 0:
 * the plain launch; otherwise the workgroups per CU and
 * *units_per_group the segments each group is cut into when run is called with segments = 0. */
int mx_nsquare_launch_timesliced(int n_bits, int64_t batch, int limbs_per_lane, int wavefronts_per_group,
                                 int* resident_per_cu, int* units_per_group);
/* The kernel INSTANCE behind that launch, for tests that must see every instance: geometry and wavefronts per group as
 * mx_nsquare_launch_shape reports them, *friendly = 1 if the tape runs modulo the friendly multiple of N (a different
 * template instance: every 3-limb one, the 9-limb two-wavefront ones for groups of 8 / 16 lanes and the 18-limb
 * one-wavefront ones for groups of 4 / 8 lanes where the modulus leaves the room), *timesliced = 1 for the time-sliced
 * form.  A friendly one-wavefront launch also runs the plain instance of the same geometry (last product, epilogue). */
/* The five-wavefront latency form (wavefronts_per_group 4) for moduli of n_bits bits (ABI 4.4): MX_ERR_SIZE where it has no
 * instance; otherwise *lanes per element (16, 32 or 64), the data *positions Pd of its rows, its *pivot (multiplier limbs on the
 * least-significant-first wavefronts: 0.52 of Pd + 3 to the nearest multiple of 3 — tools/bipair_model.py: pair_geometry) and the
 * largest batch (*max_batch: one workgroup per compute unit of the current device) for which mx_powmod_nsquare_run takes
 * the form by itself.  Any of the pointers may be NULL. */
int mx_nsquare_latency_form(int n_bits, int* lanes, int* positions, int* pivot, int64_t* max_batch);
int mx_nsquare_launch_instance(int n_bits, int64_t batch, int limbs_per_lane, int wavefronts_per_group,
                               int* lanes_per_element, int* limbs_per_lane_out, int* wavefronts_per_group_out,
                               int* friendly, int* timesliced);
/* For callers that own a second stream: whether ONE batch is better run as two launches side by side — the first
 * *first_rows elements in the shape (*first_lpl, *first_wpg), the rest in (*rest_lpl, *rest_wpg) on another stream at the
 * same time (each with its own workspace; mx_powmod_nsquare_run with explicit shapes).  *first_rows = 0: no split.
 * Since ABI 4.1 the library reports a split only when MX_KNOB_N2_SPLIT = 2 asks for it (then for every batch between
 * one and two capacities of the wide two-wavefront shape — 8192 ciphertexts at key_length 2048): the time-sliced wide
 * launch covers 8192 .. 12 288 ciphertexts in 36-48 ms, as fast as or faster than the split (48.5).  The library itself
 * never uses a stream the caller did not pass; protocols/distributed_keygen_amd/engine.py follows this hint. */
int mx_nsquare_launch_split(int n_bits, int64_t batch, int64_t* first_rows, int* first_lpl, int* first_wpg,
                            int* rest_lpl, int* rest_wpg);
/* Launch form of a generic-modulus modexp (mx_powmod_shared_lpl / mx_powmod_multi_dev) for this limbs_per_lane (0 = the
 * library's choice): *wavefronts_per_group = 1, or 2 for the BIPARTITE latency form (limbs_per_lane 6 = "3 limbs per lane on
 * two wavefronts", csrc/mx_bimont.hpp): every modular product is split at a pivot — *pivot multiplier limbs on a wavefront that
 * runs least-significant-first Montgomery steps, the rest on a second wavefront that runs most-significant-first steps with a
 * fold of the overflow — so that a product costs half the dependent limb steps plus a hand-over through LDS.  For launches that
 * leave SIMDs idle (a key-generation round at the reference's batch sizes: a few dozen to a thousand modexps,
 * distributed_keygen.py:1313-1329): such a launch lasts as long as one wavefront's dependent chain whatever its size.  Fixed
 * windows; moduli up to 5359 bits; mx_powmod_geometry_for reports its lanes per element with limbs_per_lane_out = 3. */
int mx_powmod_launch_form(int mod_bits, int64_t batch, int64_t groups, int limbs_per_lane, int* wavefronts_per_group, int* pivot);
int mx_powmod_geometry_for(int mod_bits, int64_t batch, int64_t groups, int limbs_per_lane, int* lanes_per_element,
                           int* limbs_per_lane_out, int* limb_bits, int* blocks);

/* ---- homomorphic linear maps: multi-exponentiation modulo N^2 (ABI 4.4, additions) --------------------------------
 *   d_out[r] = prod_{t < terms} d_inputs[d_index[r][t]] ^ w[r][t]  mod N^2,   w[r][t] >= 0
 * with the modulus of a plan of mx_powmod_nsquare_prepare (its constants; the plan's exponent is not used).  Interleaved
 * fixed-window (Straus) form on the pair arithmetic (csrc/mx_multiexp_n2.hpp): a table pass writes 2^window powers of
 * every input into the workspace, then one group of lanes per output squares once per window bit and multiplies once
 * per term and window.  Rows of the same launch execute the same number of terms and windows: pad with weight 0.
 *   d_inputs: [n_inputs][limbs2] residues < N^2; NULL = the tables already in the workspace (an earlier run with the
 *             same inputs, window and workspace on the same stream)
 *   d_index:  [n_outputs][terms] int32 in [0, n_inputs);  d_weights: [n_outputs][terms][(weight_bits + 31) / 32] words
 *   weight_bits <= 2 * bits(N) + 64 (weights below 2^(bits(N^2) + 64)); window 1 .. 8 (mx_multiexp_nsquare_shape).
 * limbs_per_lane: 9 (the narrow geometry: every modulus of the pair kernel with groups of up to 32 lanes) or 0.
 * Results are canonical residues in [0, N^2), NOT fresh ciphertexts: re-randomise before they leave the party. */
int mx_multiexp_nsquare_shape(int n_bits, int64_t n_inputs, int64_t n_outputs, int64_t terms, int weight_bits,
                              int limbs_per_lane, int window, int* lanes, int* limbs_per_lane_out, int* window_out,
                              int64_t* chunk_terms);
int64_t mx_multiexp_nsquare_workspace_bytes(int n_bits, int64_t n_inputs, int limbs_per_lane, int window);
int mx_multiexp_nsquare_run(const mx_nsquare_plan* plan, const uint32_t* d_inputs, int64_t n_inputs, int limbs2,
                            const int32_t* d_index, const uint32_t* d_weights, int terms, int weight_bits,
                            uint32_t* d_out, int64_t n_outputs, int limbs_per_lane, int window, void* d_workspace,
                            int64_t workspace_bytes, void* stream);
/* The kernel instances mx_multiexp_nsquare_run can select: (lanes per element, limbs per lane) pairs, at most
 * max_entries written; returns their number. */
int mx_multiexp_nsquare_instances(int* lanes, int* limbs_per_lane, int max_entries);

/* ---- encrypted matrix products over a batch of ciphertext vectors (ABI 4.4, additions) ---------------------------
 *   d_out[b][j] = prod_{t < terms} T(d_index[j][t], b) ^ w[j][t]  mod N^2,   w[j][t] >= 0,  j < n_rows,  b < tile_batch
 * — the multi-exponentiation above with the weight rows SHARED by every sample of a tile (csrc/mx_matmul_n2.hpp): the
 * same table pass over n_cols * tile_batch + n_shared inputs, then one group of lanes per (weight row, sample), the
 * groups of a wavefront being consecutive samples of one row.  d_index and d_weights are per WEIGHT ROW, never per sample.
 *   d_inputs:  [n_cols * tile_batch + n_shared][limbs2] residues < N^2: row c * tile_batch + b is table column c of
 *              sample b (column-major), followed by the n_shared rows that do not depend on the sample (the bias inputs
 *              1 + (b_j mod N) N), stored once.  NULL = the tables already in the workspace (an earlier run with the same
 *              inputs, n_cols, n_shared, tile_batch, window and workspace on the same stream)
 *   d_index:   [n_rows][terms] int32: a value c >= 0 names table column c (read at the sample's offset), a value
 *              s < 0 names the shared table -1 - s (read without it);  d_weights: [n_rows][terms][(weight_bits + 31) / 32]
 *   d_out:     [tile_batch][n_rows][limbs2], sample-major
 * A digit that is zero costs no multiplication.  THE WEIGHTS MUST BE PUBLIC: the kernel's control flow depends on them.
 * The shape query: the window of the cost model above for ONE sample (n_inputs = n_cols, n_outputs = n_rows; `window`
 * > 0 overrides it), lowered until one sample's tables fit table_budget_bytes; *tile_batch = the largest sample count
 * <= batch whose per-sample tables fit (at least 1); *chunk_terms = the split-K rule above for n_rows * *tile_batch
 * outputs.  MX_ERR_ARG for a null pointer, a zero or negative size, window outside 1 .. 8 (0 .. 8 in the shape query),
 * weight_bits above 2 * bits(N) + 64, or rows too narrow for N^2; MX_ERR_SIZE outside the narrow geometry (limbs_per_lane 9
 * or 0, groups of up to 32 lanes), for n_cols, n_rows or terms above 2^31, or beyond one grid; MX_ERR_WORKSPACE for a workspace below the query's size.  Everything
 * is checked before anything is enqueued.  Results are canonical residues in [0, N^2), NOT fresh ciphertexts. */
int mx_matmul_nsquare_shape(int n_bits, int64_t n_cols, int64_t n_rows, int64_t terms, int weight_bits, int64_t batch,
                            int64_t table_budget_bytes, int limbs_per_lane, int window, int* lanes,
                            int* limbs_per_lane_out, int* window_out, int64_t* tile_batch, int64_t* chunk_terms);
int64_t mx_matmul_nsquare_workspace_bytes(int n_bits, int64_t n_cols, int64_t n_shared, int64_t tile_batch,
                                          int limbs_per_lane, int window);
int mx_matmul_nsquare_run(const mx_nsquare_plan* plan, const uint32_t* d_inputs, int64_t n_cols, int64_t n_shared,
                          int64_t tile_batch, int limbs2, const int32_t* d_index, const uint32_t* d_weights, int terms,
                          int weight_bits, uint32_t* d_out, int64_t n_rows, int limbs_per_lane, int window,
                          void* d_workspace, int64_t workspace_bytes, void* stream);
/* The kernel instances mx_matmul_nsquare_run can select: (lanes per element, limbs per lane) pairs, at most max_entries
 * written; returns their number. */
int mx_matmul_nsquare_instances(int* lanes, int* limbs_per_lane, int max_entries);

/* ---- encrypted convolutions of ciphertext grids with a public kernel (ABI 4.4, additions) -------------------------
 *   d_out[m][j][q] = prod_{t < terms} T(d_index[j][t], b) ^ w[j][t]  mod N^2,   w[j][t] >= 0,  j < n_rows,
 *   b = m * image_positions + q < n_positions
 * — the shared-weight product above with the address rule of a sliding window (csrc/mx_matmul_n2.hpp, the same
 * kernel): the tables are the PIXELS of the padded input grids, one table each however many windows cover it, and term
 * t of position b reads
 *   T(i, b) = table i + d_origin[b]        for i >= 0  (i: the table of the tap at output position 0)
 *           = table n_local + (-1 - i)     for i <  0  (a shared table — the bias inputs 1 + (b_j mod N) N — read
 *                                                       without the origin)
 * Stride, dilation, channels and padding are in d_index and d_origin alone.  The same table pass over n_local + n_shared
 * inputs, then one group of lanes per (weight row, position), the groups of a wavefront being consecutive positions of
 * one row.
 *   d_inputs:  [n_local + n_shared][limbs2] residues < N^2 (a padded pixel is the residue 1).  NULL = the tables
 *              already in the workspace (an earlier run with the same inputs, counts, window and workspace on the same
 *              stream)
 *   d_index:   [n_rows][terms] int32;  d_weights: [n_rows][terms][(weight_bits + 31) / 32];  d_origin: [n_positions] int64
 *   THE CALLER guarantees 0 <= d_index[j][t] + d_origin[b] < n_local for every term with a non-zero weight (the arrays
 *   are device memory: the library cannot read them before the launch); the kernel clamps every table address into the
 *   table set, so a wrong array gives wrong values, never an access outside the workspace.
 *   d_out:     [n_positions / image_positions][n_rows][image_positions][limbs2]; image_positions divides n_positions.
 *              With the kernels as rows and whole images per launch that is the layout [image][kernel][y][x].
 * A digit that is zero costs no multiplication.  THE WEIGHTS MUST BE PUBLIC: the kernel's control flow depends on them.
 * No cost model of its own: a tile is a linear map of n_local + n_shared inputs and n_rows * n_positions outputs —
 * window and split-K chunk are those of mx_multiexp_nsquare_shape.
 * MX_ERR_ARG for a null pointer, a zero or negative size, no table at all, n_positions above 2^30 or no multiple of
 * image_positions, window outside 1 .. 8, weight_bits above 2 * bits(N) + 64, or rows too narrow for N^2; MX_ERR_SIZE
 * outside the narrow geometry (limbs_per_lane 9 or 0, groups of up to 32 lanes) or beyond one grid; MX_ERR_WORKSPACE for a
 * workspace below the query's size.  Everything is checked before anything is enqueued.  Results are canonical residues
 * in [0, N^2), NOT fresh ciphertexts. */
int64_t mx_conv_nsquare_workspace_bytes(int n_bits, int64_t n_local, int64_t n_shared, int limbs_per_lane, int window);
int mx_conv_nsquare_run(const mx_nsquare_plan* plan, const uint32_t* d_inputs, int64_t n_local, int64_t n_shared,
                        int limbs2, const int32_t* d_index, const uint32_t* d_weights, int terms, int weight_bits,
                        const int64_t* d_origin, int64_t n_positions, int64_t image_positions, uint32_t* d_out,
                        int64_t n_rows, int limbs_per_lane, int window, void* d_workspace, int64_t workspace_bytes,
                        void* stream);
/* The kernel instances mx_conv_nsquare_run can select: (lanes per element, limbs per lane) pairs, at most max_entries
 * written; returns their number. */
int mx_conv_nsquare_instances(int* lanes, int* limbs_per_lane, int max_entries);

/* ---- encrypted histograms: sums of ciphertexts by a public bin index (ABI 4.4, additions) ------------------------
 *   H[s] = prod_{i : segment(i) == s} c_i  mod N^2          (an empty segment gives 1)
 * — weight-1 products only (csrc/mx_hist_n2.hpp): no weights, windows, squarings or inversions, so a ciphertext
 * without an inverse modulo N^2 is a legal input.  Three steps, all on the pair arithmetic of the plan's modulus:
 *   convert:    one group of lanes per ciphertext writes its pair-form ROW (*row_bytes = 2 * lanes * limbs_per_lane * 4
 *               bytes, the layout of one table entry of the multi-exponentiation) once; row n_samples is the value one.
 *   accumulate: one group of lanes per PIECE: d_index[piece][0 .. chunk) names `chunk` rows, whose product is the
 *               piece.  Every piece of a launch has the same `chunk`: the caller cuts a segment of len terms into
 *               ceil(len / chunk) pieces and pads the last one with n_rows, the index of the one row.
 *   combine:    the same entry point over the piece rows of the level before: with pair_form_out != 0 a run writes its
 *               n_pieces products in pair form, followed by the one row, i.e. exactly the d_rows (n_rows = n_pieces) of
 *               the next run.  The last run (pair_form_out == 0) writes canonical residues in [0, N^2), n_pieces rows
 *               of limbs2 words, NOT fresh ciphertexts.
 *   d_inputs: [n_samples][limbs2] residues < N^2;  d_rows: [n_rows + 1] pair-form rows (the last one the one row);
 *   d_index:  [n_pieces][chunk] int32 in [0, n_rows] — device memory the library cannot read before the launch: the
 *             kernel clamps every index into the row set, so a wrong array gives wrong values, never an access outside
 *             d_rows;  chunk 1 .. 65536.
 * The shape query: the geometry, the row size and the library's chunk for n_segments segments of total_terms terms
 * (enough pieces to fill the device, at least 16 and at most 4096 terms each, and never more than the mean segment length
 * total_terms / n_segments rounded up — segments are padded to whole pieces; `chunk` > 0 overrides it); n_samples is
 * informative.  mx_histogram_nsquare_workspace_bytes: the bytes of a row set of n_rows rows and its one
 * row — the size of d_rows (rows_bytes) for a conversion of n_rows samples and of d_out (out_bytes) for a run with
 * pair_form_out over n_rows pieces; a run without it needs n_pieces * limbs2 * 4 bytes.
 * MX_ERR_ARG for a null pointer, a zero or negative size, a chunk outside 1 .. 65536 (0 .. 65536 in the shape query),
 * a limbs_per_lane other than 9 or 0, or rows too narrow for N^2; MX_ERR_SIZE outside the narrow geometry (groups of up
 * to 32 lanes) or beyond one grid; MX_ERR_WORKSPACE for rows_bytes / out_bytes below the sizes above.  Everything is
 * checked before anything is enqueued. */
int mx_histogram_nsquare_shape(int n_bits, int64_t n_samples, int64_t n_segments, int64_t total_terms, int limbs_per_lane,
                               int chunk, int* lanes, int* limbs_per_lane_out, int* chunk_out, int64_t* row_bytes);
int64_t mx_histogram_nsquare_workspace_bytes(int n_bits, int64_t n_rows, int limbs_per_lane);
int mx_histogram_nsquare_convert(const mx_nsquare_plan* plan, const uint32_t* d_inputs, int64_t n_samples, int limbs2,
                                 uint32_t* d_rows, int64_t rows_bytes, int limbs_per_lane, void* stream);
int mx_histogram_nsquare_run(const mx_nsquare_plan* plan, const uint32_t* d_rows, int64_t n_rows, const int32_t* d_index,
                             int64_t n_pieces, int chunk, uint32_t* d_out, int pair_form_out, int limbs2,
                             int64_t out_bytes, int limbs_per_lane, void* stream);
/* The kernel instances mx_histogram_nsquare_convert / _run can select: (lanes per element, limbs per lane) pairs, at
 * most max_entries written; returns their number. */
int mx_histogram_nsquare_instances(int* lanes, int* limbs_per_lane, int max_entries);

/* ---- encrypted prefix sums: running totals over series of ciphertexts (ABI 4.4, additions) -----------------------
 *   out[index[piece][t]] = carry(piece) * prod_{u <= t} rows[index[piece][u]]  mod N^2      (inclusive)
 *   out[index[piece][t]] = carry(piece) * prod_{u <  t} rows[index[piece][u]]  mod N^2      (exclusive != 0)
 * — the accumulate step of the histogram with every intermediate product stored (csrc/mx_scan_n2.hpp): the same
 * pair-form rows (mx_histogram_nsquare_convert writes them), the same index array, weight-1 products only, so a
 * ciphertext without an inverse modulo N^2 is a legal input.
 *   d_rows:   [n_rows + 1] pair-form rows, the last one the one row;
 *   d_index:  [n_pieces][chunk] int32 in [0, n_rows]: one group of lanes per PIECE walks its `chunk` terms in order.
 *             The product of a term is stored at the OUTPUT row of the term's own number, so every row should be named
 *             once (a reverse scan is a reversed index array); a term that names n_rows, the padding of a piece,
 *             stores nothing.  chunk 1 .. 65536;
 *   carry:    d_carry_rows, a second row set of n_carry_rows rows and its one row, and d_carry_index[n_pieces] int32 in
 *             [0, n_carry_rows]: what a piece starts from — the product of everything before it in its segment.  With
 *             d_carry_rows null every piece starts from one, and n_carry_rows and d_carry_index are ignored;
 *   d_out:    a row set of n_rows rows followed by the one row (out_bytes at least what
 *             mx_histogram_nsquare_workspace_bytes gives for n_rows), i.e. the d_rows or d_carry_rows of another run or
 *             the d_rows of the store.  A row that no term names is left as it was.
 * mx_scan_nsquare_store writes the n_rows rows of a row set as canonical residues in [0, N^2), n_rows rows of limbs2
 * words (out_bytes at least n_rows * limbs2 * 4), NOT fresh ciphertexts.  It is a pass of its own because the epilogue
 * does not fit beside the accumulator inside the scan loop without spilling registers.
 * Both index arrays are device memory the library cannot read before the launch: the kernel clamps every entry into its
 * row set, so a wrong array gives wrong values, never an access outside d_rows, d_carry_rows or d_out.  The caller builds
 * running totals over segments longer than one piece in levels: piece totals by mx_histogram_nsquare_run over the same
 * index array, their exclusive scan by this entry point one level up, then the scan of the level with those carries.
 * The geometry, the row size and the library's chunk are those of mx_histogram_nsquare_shape.
 * MX_ERR_ARG for a null pointer (a null carry set is legal; with one, d_carry_index is required), a zero or negative
 * size (n_carry_rows may be 0), a chunk outside 1 .. 65536, a limbs_per_lane other than 9 or 0, or rows too narrow for
 * N^2; MX_ERR_SIZE outside the narrow geometry (groups of up to 32 lanes) or beyond one grid; MX_ERR_WORKSPACE for an
 * out_bytes below the sizes above.  Everything is checked before anything is enqueued. */
int mx_scan_nsquare_run(const mx_nsquare_plan* plan, const uint32_t* d_rows, int64_t n_rows, const int32_t* d_index,
                        int64_t n_pieces, int chunk, const uint32_t* d_carry_rows, int64_t n_carry_rows,
                        const int32_t* d_carry_index, int exclusive, uint32_t* d_out, int limbs2, int64_t out_bytes,
                        int limbs_per_lane, void* stream);
int mx_scan_nsquare_store(const mx_nsquare_plan* plan, const uint32_t* d_rows, int64_t n_rows, uint32_t* d_out, int limbs2,
                          int64_t out_bytes, int limbs_per_lane, void* stream);
/* The kernel instances mx_scan_nsquare_run / _store can select: (lanes per element, limbs per lane) pairs, at most
 * max_entries written; returns their number. */
int mx_scan_nsquare_instances(int* lanes, int* limbs_per_lane, int max_entries);

/* ---- encrypted sparse matrix products: a public CSR matrix over ciphertexts (ABI 4.4, additions) -----------------
 *   y_r = bias_r * prod_{t in row r} x_{col[t]} ^ |val[t]|  mod N^2        (a negative weight: the caller hands in the inverse)
 * as a histogram over windowed digits (csrc/mx_spmm_n2.hpp).  With window w and weights below 2^weight_bits there are
 * D = ceil(weight_bits / w) digit positions; every non-zero digit d of a term at position p is a weight-1 term of the
 * segment r * D + p which names the table row of x^d.  The caller builds the index arrays; the library has the two
 * kernels on either side of mx_histogram_nsquare_run:
 *   tables: one group of lanes per input writes x^1 .. x^(2^w - 1) in pair form as rows of a histogram row set: entry
 *           (input i, digit d) is row i * (2^w - 1) + d - 1, the one row follows the last entry, so the result is the
 *           d_rows (n_rows = n_inputs * (2^w - 1)) of mx_histogram_nsquare_run.  rows_bytes at least what
 *           mx_spmm_nsquare_workspace_bytes gives for (n_inputs, window).  With window 1 this is the conversion alone.
 *   horner: d_rows is a row set of n_rows * positions rows (row r * positions + p the product of segment (r, p): the
 *           output of a run with pair_form_out).  One group of lanes per output row: acc = S[r][positions - 1], then
 *           for p = positions - 2 .. 0 `window` pair squarings and one pair product by S[r][p]; then one product by
 *           d_bias_rows[r] — n_rows pair-form rows, e.g. mx_histogram_nsquare_convert of the residues 1 + b_r N — unless
 *           it is null; n_rows canonical residues in [0, N^2) of limbs2 words (out_bytes at least n_rows * limbs2 * 4),
 *           NOT fresh ciphertexts.  Trip counts depend on (positions, window) alone.
 * The shape query needs no GPU: the geometry, the row size, the window and the positions for n_tables tables (the
 * inputs plus the inverted columns), n_rows output rows and nnz stored terms of weights below 2^weight_bits.  The window
 * minimises   n_tables (2^w - 2) + nnz ceil(weight_bits / w) + n_rows (ceil(weight_bits / w) - 1) (w + 1)   over
 * w = 1 .. 6, ties to the smaller w; `window` 1 .. 8 overrides it.  *positions = max(1, ceil(weight_bits / window)).
 * The chunk of the index arrays is mx_histogram_nsquare_shape's, for the digit terms and n_rows * positions segments.
 * MX_ERR_ARG for a null pointer, a negative count, n_inputs / n_rows / positions < 1, weight_bits outside 0 .. 63,
 * positions above 64, a window outside 1 .. 8 (0 .. 8 in the shape query), a row count of 2^31 - 1 or more, a
 * limbs_per_lane other than 9 or 0, or rows too narrow for N^2; MX_ERR_SIZE outside the narrow geometry (groups of up
 * to 32 lanes) or beyond one grid; MX_ERR_WORKSPACE for rows_bytes / out_bytes below the sizes above.  Everything is
 * checked before anything is enqueued. */
int mx_spmm_nsquare_shape(int n_bits, int64_t n_tables, int64_t n_rows, int64_t nnz, int weight_bits, int limbs_per_lane,
                          int window, int* lanes, int* limbs_per_lane_out, int* window_out, int* positions,
                          int64_t* row_bytes);
int64_t mx_spmm_nsquare_workspace_bytes(int n_bits, int64_t n_inputs, int window, int limbs_per_lane);
int mx_spmm_nsquare_tables(const mx_nsquare_plan* plan, const uint32_t* d_inputs, int64_t n_inputs, int limbs2, int window,
                           uint32_t* d_rows, int64_t rows_bytes, int limbs_per_lane, void* stream);
int mx_spmm_nsquare_horner(const mx_nsquare_plan* plan, const uint32_t* d_rows, int64_t n_rows, int positions, int window,
                           const uint32_t* d_bias_rows, uint32_t* d_out, int limbs2, int64_t out_bytes, int limbs_per_lane,
                           void* stream);
/* The kernel instances mx_spmm_nsquare_tables / _horner can select: (lanes per element, limbs per lane) pairs, at most
 * max_entries written; returns their number. */
int mx_spmm_nsquare_instances(int* lanes, int* limbs_per_lane, int max_entries);

/* ---- packing: many small plaintexts per ciphertext (ABI 4.4, additions) ------------------------------------------
 *   d_out[j] = prod_{i < slots} d_cts[j * slots + i] ^ (2^(slot_bits * i))  mod N^2,   j < ceil(count / slots)
 * which encrypts sum_i m_i 2^(slot_bits i) when every d_cts[r] encrypts m_r (g = N + 1): one threshold decryption of
 * d_out[j] returns `slots` plaintexts of slot_bits bits.  Rows at index count or above count as 1 (the last output may
 * hold fewer slots).  Horner on the pair arithmetic with the constants of a plan of mx_powmod_nsquare_prepare (its
 * exponent is not used): (slots - 1) * slot_bits pair squarings per output (csrc/mx_pack_n2.hpp).  Enqueues only, on
 * `stream`, no workspace; writes ceil(count / slots) rows of limbs2 words.
 *   d_cts: [count][limbs2] residues < N^2 (any residue: 0 and multiples of N included, nothing is inverted)
 *   MX_ERR_ARG for a null pointer, count / slots / slot_bits < 1, slot_bits * slots > bits(N) - 2 (the bound under
 *   which a signed or unsigned packed plaintext decrypts unambiguously) or rows too narrow for N^2;
 *   MX_ERR_SIZE outside the narrow geometry (limbs_per_lane 9 or 0, groups of up to 32 lanes).
 * Results are canonical residues in [0, N^2), NOT fresh ciphertexts. */
int mx_pack_nsquare_run(const mx_nsquare_plan* plan, const uint32_t* d_cts, int64_t count, int limbs2, int slot_bits,
                        int slots, uint32_t* d_out, int limbs_per_lane, void* stream);
/* The kernel instances mx_pack_nsquare_run can select: (lanes per element, limbs per lane) pairs, at most max_entries
 * written; returns their number. */
int mx_pack_nsquare_instances(int* lanes, int* limbs_per_lane, int max_entries);

/* ---- slot-packed plaintexts: the codec between int64 values and plaintext rows (ABI 4.4, additions) ---------------
 * The layout of the packing above, produced BEFORE encryption: value j * slots + i occupies bits
 * [slot_bits * i, slot_bits * (i + 1)) of plaintext j, j < ceil(count / slots); the last plaintext holds the remaining
 * values, its missing slots count as 0 (csrc/mx_slots.hpp).
 *   is_signed != 0: values in [-2^(slot_bits-1), 2^(slot_bits-1)), slot_bits 1 .. 64; plaintext j is
 *                   (sum_i m_(j slots + i) 2^(slot_bits i)) mod N, and decode reads a residue v > N div 2 as v - N
 *   is_signed == 0: values in [0, 2^slot_bits), slot_bits 1 .. 63
 * mx_slots_encode writes d_out [ceil(count / slots)][out_stride] rows — the canonical residue in [0, N) in the first
 * limbs_n words, zeros beyond — and d_status [ceil(count / slots)]: 1 if any value of that plaintext lies outside the
 * slot range (its row is then unspecified), else 0.  These rows are what mx_fixedbase_nsquare_run takes as the operand
 * of MX_FIXEDBASE_ENCRYPT.
 * mx_slots_decode reads d_rows [ceil(count / slots)][row_stride] residues in [0, N) — words at limbs_n and beyond are
 * ignored, so the rows of mx_combine_run with out_stride = limbs + 1 are taken as they are — and writes d_out [count].
 * Any residue decodes: fields are extracted from ((v or v - N) + offset) mod 2^(slot_bits * slots), so values that had
 * overflowed their slots come out as they would from the same arithmetic on integers.
 *   h_n: limbs_n HOST words, travelling by value in the kernel-argument block (limbs_n <= 258, MX_ERR_SIZE beyond).
 *   MX_ERR_ARG for a null pointer, count < 0, slots < 1, slot_bits outside its range, slot_bits * slots > bits(N) - 2
 *   or a stride below limbs_n; MX_ERR_MODULUS for an even N.  count = 0 returns MX_OK without a launch.  One launch on
 *   `stream`, no workspace, no synchronisation. */
int mx_slots_encode(const int64_t* d_values, int64_t count, const uint32_t* h_n, int limbs_n, int slot_bits, int slots,
                    int is_signed, uint32_t* d_out, int out_stride, uint8_t* d_status, void* stream);
int mx_slots_decode(const uint32_t* d_rows, int row_stride, int64_t count, const uint32_t* h_n, int limbs_n,
                    int slot_bits, int slots, int is_signed, int64_t* d_out, void* stream);

/* ---- fixed-base exponentiation: encryption and re-randomisation (ABI 4.4, additions) -------------------------------
 *   d_out[r] = f_r * g^(e_r)  mod N^2,   r < count,   ONE base g per table, exponents e_r < 2^exp_bits
 * with the constants of a plan of mx_powmod_nsquare_prepare (its exponent is not used).  mx_fixedbase_nsquare_prepare
 * tabulates g^(d 2^(window i)) for every window i < ceil(exp_bits / window) and digit d < 2^window in pair form
 * (csrc/mx_fixedbase_n2.hpp: a chain of exp_bits squarings on one group, then every further entry on a group of its
 * own) into caller-owned device memory; mx_fixedbase_nsquare_run then costs ceil(exp_bits / window) pair products per
 * output and NO squaring.  A table serves any number of runs, on any stream ordered after the prepare.
 *   mode MX_FIXEDBASE_POWER      f_r = 1                        d_operand NULL
 *        MX_FIXEDBASE_ENCRYPT    f_r = 1 + m_r N                d_operand [count][operand_limbs] messages m_r < N
 *        MX_FIXEDBASE_RANDOMIZE  f_r = c_r                      d_operand [count][operand_limbs] residues c_r < N^2
 *   d_base:  [limbs2] any residue < N^2 (0 and multiples of N included: nothing is inverted)
 *   d_exps:  [count][(exp_bits + 31) / 32] little-endian words; bits at exp_bits and above are ignored
 *   exp_bits 1 .. 2 * bits(N) + 64; window 1 .. 8 (mx_fixedbase_nsquare_shape: the window that minimises the run's
 *   products for `count` outputs plus a sixteenth of the table pass — a table is built once per key and serves many
 *   calls — among the tables of at most table_budget_bytes, 0 = 256 MiB; an explicit window is taken as given;
 *   *windows = ceil(exp_bits / *window)).
 *   MX_ERR_ARG for a null pointer, count < 1, exp_bits or window out of range, a table buffer smaller than
 *   mx_fixedbase_nsquare_table_bytes, a missing operand, rows too narrow for N^2 (for N: ENCRYPT's operand);
 *   MX_ERR_SIZE outside the narrow geometry (limbs_per_lane 9 or 0, groups of up to 32 lanes).  A refused call launches
 *   nothing.  Enqueue only, on `stream`, no workspace.  Results are canonical residues in [0, N^2). */
#define MX_FIXEDBASE_POWER 0
#define MX_FIXEDBASE_ENCRYPT 1
#define MX_FIXEDBASE_RANDOMIZE 2
int mx_fixedbase_nsquare_shape(int n_bits, int exp_bits, int64_t count, int64_t table_budget_bytes, int limbs_per_lane,
                               int window, int* lanes, int* limbs_per_lane_out, int* window_out, int* windows);
int64_t mx_fixedbase_nsquare_table_bytes(int n_bits, int exp_bits, int limbs_per_lane, int window);
int mx_fixedbase_nsquare_prepare(const mx_nsquare_plan* plan, const uint32_t* d_base, int limbs2, int exp_bits,
                                 int limbs_per_lane, int window, void* d_table, int64_t table_bytes, void* stream);
int mx_fixedbase_nsquare_run(const mx_nsquare_plan* plan, const void* d_table, int exp_bits, int window, int mode,
                             const uint32_t* d_exps, const uint32_t* d_operand, int operand_limbs, uint32_t* d_out,
                             int64_t count, int limbs2, int limbs_per_lane, void* stream);
/* The kernel instances the fixed-base entries can select: (lanes per element, limbs per lane) pairs, at most
 * max_entries written; returns their number. */
int mx_fixedbase_nsquare_instances(int* lanes, int* limbs_per_lane, int max_entries);

/* ---- random rows on the device: ChaCha20 keystream (ABI 4.4, additions) -------------------------------------------
 *   d_out[r][j] = keystream word r * w + j,   r < count, j < w = ceil(bits / 32)
 * of ChaCha20 as RFC 8439 specifies it (csrc/mx_chacha.hpp; tools/chacha_model.py is the bit-exact model): state = four
 * constants, the eight key words, a 32-bit block counter in word 12, the three nonce words in words 13-15; twenty rounds
 * and the feed-forward addition; output words in state order.  Keystream word i is word i mod 16 of block
 * counter0 + i div 16.  The top word of every row is masked to bits mod 32 bits when that is not 0, words
 * w .. row_words - 1 of every row are written as 0, and the unused tail of the last block is discarded (never carried into
 * another call).  The mapping does not depend on the launch shape.  These rows are what mx_fixedbase_nsquare_run takes as
 * d_exps and, at the width of N^2, what mx_powmod_nsquare_run takes as bases: exponents and randomness r without a host
 * draw and an upload.
 *   key, nonce: HOST arrays that travel by value in the kernel-argument block (they may be freed or overwritten on
 *   return).  The caller owns the discipline that makes the stream unpredictable: a secret uniform key, and no
 *   (key, nonce, block counter) triple used twice.
 *   One launch on `stream`, no workspace, no synchronisation; count = 0 returns MX_OK without a launch.
 *   MX_ERR_ARG for a null pointer, count < 0, bits < 1, bits > 32 * row_words, or a request whose blocks do not fit the
 *   counter: counter0 + ceil(count * w / 16) > 2^32.  A refused call launches nothing. */
int mx_chacha20_rows(const uint32_t key[8], const uint32_t nonce[3], uint32_t counter0, uint32_t* d_out, int64_t count,
                     int row_words, int bits, void* stream);

/* ---- additive shares of the prime candidates and their Shamir sharings (ABI 4.4, additions) ------------------------
 * The step of a key-generation round in front of the candidate moduli (`_generate_pq`, DK:718-853), for all candidates
 * of the round at once (csrc/mx_share.hpp; tools/share_model.py is the model).
 *
 * mx_share_candidates: d_out[e] = 2^(L-1) + (d_random[e] << 2) + m4 with L = prime_length and m4 = 3 when first_party
 *   is non-zero, else 0 (DK:874-875).  d_random is [count][ceil((L - 3) / 32)], rows of L - 3 random bits (zero above
 *   them: what mx_chacha20_rows writes for bits = L - 3); d_out is [count][row_words], zero above bit L - 1.  One launch,
 *   no workspace; count = 0 returns MX_OK without a launch.  MX_ERR_ARG for a null pointer, count < 0, prime_length < 8
 *   or row_words < 1; MX_ERR_SIZE for prime_length > 32 * row_words.
 *
 * mx_shamir_share: d_out[j][e] = s[e] + sum_{k=1..degree} (D[k][e] mod P) * x_j^k mod P, canonical residues —
 *   `ShamirVariable.share()` (UT:253-260) of every candidate: the values at the public points x_j = h_points[j] of a
 *   polynomial of degree `degree` whose constant term is the secret and whose coefficients are the draws reduced modulo
 *   P = h_mod.  d_secrets is [batch][limbs] with every row below P, or NULL for a sharing of zero; d_draws is
 *   [degree][batch][cw] with cw = ceil((bits(P) + 64) / 32): draws of bits(P) + 64 bits (a coefficient is then uniform
 *   on [0, P) up to a bias below 2^-64); d_out is [n_points][batch][limbs], the layout mx_lincomb_mod reads.  One
 *   modulus per launch; control flow and addresses depend on the sizes alone.
 *   MX_ERR_ARG for a null pointer (other than d_secrets), limbs, batch or degree < 1, n_points <= degree, or points that
 *   are not distinct values in [1, 2^16); MX_ERR_MODULUS for an even P; MX_ERR_SIZE for a P beyond the engine's widest
 *   modulus or degree > MX_SHARE_MAX_DEGREE (the coefficients of an element are kept in LDS); MX_ERR_WORKSPACE below
 *   mx_share_workspace_bytes.  A refused call launches nothing. */
#define MX_SHARE_MAX_DEGREE 24
int mx_share_candidates(const uint32_t* d_random, uint32_t* d_out, int64_t count, int prime_length, int first_party,
                        int row_words, void* stream);
int64_t mx_share_workspace_bytes(int limbs, int n_points);
int mx_shamir_share(const uint32_t* d_secrets, const uint32_t* d_draws, const uint32_t* h_points, int n_points, int degree,
                    uint32_t* d_out, const uint32_t* h_mod, int limbs, int64_t batch, void* d_workspace,
                    int64_t workspace_bytes, void* stream);

/* ---- jointly random generators of the biprimality test (ABI 4.4, additions) ----------------------------------------
 * The generator step of a key-generation round (`__biprime_test_g_generation`, DK:1001-1054) for all survivors of the
 * sieve at once: `groups` candidate moduli N_c, `group_size` generators each, row c * group_size + k belongs to
 * generator k of candidate c (csrc/mx_generators.hpp; tools/generators_model.py is the model).  The moduli are DEVICE
 * rows d_mods [groups][limbs] of at most mod_bits bits, as for mx_powmod_multi_dev (the survivors' moduli stay on the
 * device from their reconstruction on); they must be odd and >= 3.  h_mods is an optional HOST copy of the same rows:
 * when it is not NULL every row is checked (MX_ERR_MODULUS for an even row, a row below 3 or one wider than mod_bits);
 * device rows alone cannot be checked — an even modulus then yields an unspecified residue for its group, never a hang.
 *
 * mx_generator_shares: d_out[r] = d_draws[r] mod N_c, canonical.  d_draws is [groups * group_size][cw] with
 *   cw = ceil((mod_bits + 64) / 32): draws of mod_bits + 64 bits (what mx_chacha20_rows writes for bits = mod_bits + 64,
 *   row_words = cw), so a share is uniform on [0, N_c) up to a bias below 2^-64; any row of cw words is reduced
 *   correctly.  d_out is [groups * group_size][limbs].
 * mx_generator_sum: d_out[r] = sum_j d_shares[j][r] mod N_c, canonical.  d_shares is [n_parties][groups * group_size]
 *   [limbs]; ANY row of `limbs` words is accepted as a share (N_c itself, unreduced values, 2^(32 limbs) - 1).  d_out has
 *   the layout mx_jacobi_dev and mx_powmod_multi_dev read.  The shares are added as unreduced columns and reduced once:
 *   the sum of their parts below 2^(mod_bits - 1), plus a residue below 2 N_c, must stay below the Montgomery radix
 *   R >= 2^(mod_bits + 4), i.e. (n_parties + 4) 2^(mod_bits - 1) <= 2^(mod_bits + 4), which holds up to 28 parties;
 *   MX_GEN_MAX_PARTIES is the power of two inside that bound.
 * Both: two launches on `stream` (the per-modulus constant R^2 mod N_c into the workspace, then the rows), no
 * synchronisation; control flow and addresses depend on the sizes alone.  groups = 0 or group_size = 0 returns MX_OK
 * without a launch.  MX_ERR_ARG for a null pointer (other than h_mods), limbs < 1, a negative count, mod_bits outside
 * [2, 32 * limbs] or n_parties outside [1, MX_GEN_MAX_PARTIES]; MX_ERR_MODULUS as above; MX_ERR_SIZE for mod_bits beyond
 * the engine's widest modulus, rows wider than the kernel stages (limbs far beyond mod_bits / 32) or more rows than a
 * launch addresses; MX_ERR_WORKSPACE below mx_generator_workspace_bytes.  A refused call launches nothing. */
#define MX_GEN_MAX_PARTIES 16
int64_t mx_generator_workspace_bytes(int limbs, int64_t groups);
int mx_generator_shares(const uint32_t* d_draws, uint32_t* d_out, const uint32_t* d_mods, const uint32_t* h_mods, int limbs,
                        int mod_bits, int64_t groups, int64_t group_size, void* d_workspace, int64_t workspace_bytes,
                        void* stream);
int mx_generator_sum(const uint32_t* d_shares, int n_parties, uint32_t* d_out, const uint32_t* d_mods, const uint32_t* h_mods,
                     int limbs, int mod_bits, int64_t groups, int64_t group_size, void* d_workspace, int64_t workspace_bytes,
                     void* stream);

/* ---- private-key (CRT) decryption (ABI 4.4, additions) ---------------------------------------------------------------
 * For the holder of an ordinary Paillier private key, who knows the primes p and q of N (Paillier 1999, section 7; never
 * the distributed key, whose primes nobody knows).  Per ciphertext c:
 *     x_p = (c mod p^2)^(p-1) mod p^2     m_p = L_p(x_p) h_p mod p     L_p(x) = (x - 1) / p
 *     x_q = (c mod q^2)^(q-1) mod q^2     m_q = L_q(x_q) h_q mod q
 *     m   = m_p + p ((m_q - m_p) p^-1 mod q)
 * The two modexps are mx_powmod_nsquare_run with plans for (n, exponent) = (p, p - 1) and (q, q - 1) — both moduli are
 * squares; the entry points here are what stands around them (csrc/mx_crt.hpp; tools/crt_model.py is the model).
 *
 * mx_crt_prepare: h_p, h_q, h_hp, h_hq, h_pinv are HOST rows of `limbs` words — the primes, h_p = L_p((N+1)^(p-1) mod
 *   p^2)^-1 mod p, h_q likewise, and p^-1 mod q (residues; the three are taken modulo their prime).  Only Montgomery
 *   constants are derived from them: no inverse, no primality test.  limbs2 is the width of the ciphertext rows, at least
 *   the words of N^2.  The plan block needs mx_crt_plan_bytes(limbs, limbs2) bytes.  limbs_half = the words of the larger
 *   of p^2 and q^2 and limbs_n = the words of N are reported in the plan.
 *     MX_ERR_ARG for a null pointer, limbs or limbs2 below 1, p == q, or rows too narrow for N^2; MX_ERR_MODULUS for an even
 *     p or q or one below 3; MX_ERR_SIZE beyond the engine's widest modulus (or limbs2 far beyond the words of N^2);
 *     MX_ERR_WORKSPACE for a plan block that is too small.  A refused call launches nothing.
 * mx_crt_split_run: d_cts [batch][limbs2], ANY value below 2^(32 limbs2) -> d_out [2][batch][limbs_half]: c mod p^2,
 *   then c mod q^2, canonical; each half is a contiguous block of rows that mx_powmod_nsquare_run takes as it is.
 * mx_crt_recombine_run: d_xp, d_xq [batch][limbs_half], x_p below p^2 and x_q below q^2 (what the modexps leave) ->
 *   d_out [batch][out_stride] and d_status [batch]: status bit 0 = x_p is not 1 modulo p, bit 1 = x_q is not 1 modulo q;
 *   m = 0 where the status is not 0, else m canonical in [0, N).  out_stride >= limbs_n; as for mx_combine_run, a wider
 *   row receives the status in word [limbs_n] and zeros behind it, and d_status may then be NULL.
 * Both runs: one launch on `stream`, no workspace, no synchronisation; control flow and addresses depend on the sizes
 * alone.  MX_ERR_ARG for a null pointer, batch < 1, out_stride below limbs_n or no place for the status; MX_ERR_SIZE for
 * more rows than a launch addresses. */
typedef struct mx_crt_plan {
  const void* d_plan;
  int64_t plan_bytes;
  int32_t limbs, limbs2, limbs_half, limbs_n, p_bits, q_bits;
} mx_crt_plan;
int64_t mx_crt_plan_bytes(int limbs, int limbs2);
int mx_crt_prepare(mx_crt_plan* plan, const uint32_t* h_p, const uint32_t* h_q, const uint32_t* h_hp, const uint32_t* h_hq,
                   const uint32_t* h_pinv, int limbs, int limbs2, void* d_plan, int64_t plan_bytes, void* stream);
int mx_crt_split_run(const mx_crt_plan* plan, const uint32_t* d_cts, uint32_t* d_out, int64_t batch, void* stream);
int mx_crt_recombine_run(const mx_crt_plan* plan, const uint32_t* d_xp, const uint32_t* d_xq, uint32_t* d_out, int out_stride,
                         uint8_t* d_status, int64_t batch, void* stream);

/* Private-key (CRT) Paillier ENCRYPTION: the noise r^N mod N^2 from half-size modexps, for the party that knows p and q.
 * Modulo p^2, x -> x^p depends on x mod p only, multiplicatively, so
 *     rho_p = r^N mod p^2 = ((r mod p)^(q mod (p-1)) mod p)^p mod p^2,     rho_q likewise,
 * and for randomness of the key holder's own, rho_p = (D mod p^2)^p, rho_q = (D mod q^2)^q of one draw D is a uniform N-th
 * residue.  The modexps are mx_powmod_shared_lpl modulo p and q and mx_powmod_nsquare_run with plans for (n, exponent) =
 * (p, p) and (q, q); the entry points here are what stands around them (csrc/mx_crt_enc.hpp; tools/crt_model.py:
 * CrtEncPlan is the model).  mx_crt_split_run reduces a draw or a ciphertext modulo the squares.
 *
 * mx_crt_enc_prepare: h_p, h_q are HOST rows of `limbs` words, h_p2inv = (p^2)^-1 mod q^2 one of 2 * limbs words.  Only
 *   Montgomery constants are derived from them.  limbs_r is the width of the randomness rows of mx_crt_prime_split_run
 *   (any width from 1).  The plan block needs mx_crt_enc_plan_bytes(limbs, limbs_r) bytes.  limbs_half, limbs_n and
 *   limbs2 = the words of N^2 are reported in the plan.
 *     MX_ERR_ARG for a null pointer, limbs or limbs_r below 1 or p == q; MX_ERR_MODULUS for an even p or q or one below 3;
 *     MX_ERR_SIZE beyond the engine's widest modulus (or limbs_r beyond what a lane group stages); MX_ERR_WORKSPACE for a
 *     plan block that is too small.  A refused call launches nothing.
 * mx_crt_prime_split_run: d_rows [batch][limbs_r], ANY value below 2^(32 limbs_r) -> d_out [2][batch][limbs_half]: r mod p,
 *   then r mod q, canonical, zero above the prime's words — rows that mx_powmod_shared_lpl takes as they are and whose
 *   results mx_powmod_nsquare_run takes as they are.
 * mx_crt_lift_run: d_rho_p, d_rho_q [batch][limbs_half], below p^2 and q^2 -> d_out [batch][out_stride], canonical in
 *   [0, N^2):  c = v rho with rho = CRT(rho_p, rho_q) and v = 1 + m N for d_messages [batch][message_stride] (m below N,
 *   message_stride >= limbs_n), v = the ciphertext whose halves d_halves [2][batch][limbs_half] holds (what
 *   mx_crt_split_run gives), or v = 1 when both are NULL.  d_status [batch]: bit 0 = rho_p is 0, bit 1 = rho_q is 0 (p or q
 *   divides the randomness); the row is zero then.  out_stride >= limbs2; as for mx_crt_recombine_run a wider row receives
 *   the status in word [limbs2] and zeros behind it, and d_status may then be NULL.
 * Both runs: one launch on `stream`, no workspace, no synchronisation; control flow and addresses depend on the sizes
 * and the mode alone.  MX_ERR_ARG for a null pointer, batch < 1, both d_messages and d_halves, message rows narrower than
 * N, out_stride below limbs2 or no place for the status; MX_ERR_SIZE for more rows than a launch addresses. */
typedef struct mx_crt_enc_plan {
  const void* d_plan;
  int64_t plan_bytes;
  int32_t limbs, limbs_r, limbs2, limbs_half, limbs_n, p_bits, q_bits;
} mx_crt_enc_plan;
int64_t mx_crt_enc_plan_bytes(int limbs, int limbs_r);
int mx_crt_enc_prepare(mx_crt_enc_plan* plan, const uint32_t* h_p, const uint32_t* h_q, const uint32_t* h_p2inv, int limbs,
                       int limbs_r, void* d_plan, int64_t plan_bytes, void* stream);
int mx_crt_prime_split_run(const mx_crt_enc_plan* plan, const uint32_t* d_rows, uint32_t* d_out, int64_t batch, void* stream);
int mx_crt_lift_run(const mx_crt_enc_plan* plan, const uint32_t* d_rho_p, const uint32_t* d_rho_q, const uint32_t* d_messages,
                    int message_stride, const uint32_t* d_halves, uint32_t* d_out, int out_stride, uint8_t* d_status,
                    int64_t batch, void* stream);

/* ---- the strong-pseudoprime (Miller-Rabin) test over a batch of candidates (ABI 4.4, additions) ----------------------
 * For the party that makes or vets an ordinary private key: `groups` odd candidates n_c >= 3 as DEVICE rows d_cands
 * [groups][limbs] of at most mod_bits bits, of any mix of lengths; n_c - 1 = 2^s d with d odd (csrc/mx_mr.hpp;
 * tools/mr_model.py is the model).  h_cands is an optional HOST copy of the same rows, checked as for mx_generator_shares
 * (MX_ERR_MODULUS for an even row, a row below 3 or one wider than mod_bits); unchecked device rows that are even yield an
 * unspecified verdict, never a hang or an access outside the rows.
 *
 * mx_mr_split: d_d [groups][limbs] = d, d_s [groups] = s (1 <= s < mod_bits).
 * mx_mr_tail:  the witness loop of `group_size` rounds per candidate.  d_x0 [groups * group_size][limbs] holds
 *   b^d mod n_c, canonical — what mx_powmod_multi_dev leaves for the bases d_bases (same shape, canonical residues), the
 *   moduli d_cands and the exponents d_d — and d_s the s of mx_mr_split.  d_pass[c * group_size + k] = 1 iff the round
 *   passes: b == 0 (a vacuous round), x0 == 1, x0 == n_c - 1, or x0^(2^i) == n_c - 1 for an i in [1, s).  The loop of a
 *   wavefront is as long as the largest s among its rows.
 * mx_mr_base2: d_pass[c] = the verdict of the round to the base 2, from the candidate alone: one squaring and one
 *   selected doubling per bit of mod_bits, no table; the sequence of operations depends on mod_bits and, for the
 *   comparisons of the last steps, on the largest s of a wavefront.
 * All three: one launch on `stream`, no workspace, no synchronisation; addresses depend on the sizes alone.  groups = 0 or
 * group_size = 0 returns MX_OK without a launch.  MX_ERR_ARG for a null pointer (other than h_cands), limbs < 1, a negative
 * count or mod_bits outside [2, 32 * limbs]; MX_ERR_MODULUS as above; MX_ERR_SIZE for mod_bits beyond the engine's widest
 * modulus, rows wider than the kernel stages (limbs far beyond mod_bits / 32) or more rows than a launch addresses.  A
 * refused call launches nothing. */
int mx_mr_split(const uint32_t* d_cands, const uint32_t* h_cands, uint32_t* d_d, int32_t* d_s, int limbs, int mod_bits,
                int64_t groups, void* stream);
int mx_mr_tail(const uint32_t* d_x0, const uint32_t* d_bases, const int32_t* d_s, uint8_t* d_pass, const uint32_t* d_cands,
               const uint32_t* h_cands, int limbs, int mod_bits, int64_t groups, int64_t group_size, void* stream);
int mx_mr_base2(const uint32_t* d_cands, const uint32_t* h_cands, uint8_t* d_pass, int limbs, int mod_bits, int64_t groups,
                void* stream);

/* ---- the safe-prime search: p = 2h + 1 with h and p prime (ABI 4.4, additions) ---------------------------------------
 * For the party that makes or vets a key of two safe primes (csrc/mx_sieve.hpp, csrc/mx_safe.hpp; tools/mr_model.py is the model).
 *
 * mx_safe_sieve: the joint sieve of h and 2h + 1 over `batch` DEVICE rows d_halves [batch][limbs] of h:  d_out[e] = 1 iff
 *   some h_primes[k] = l has h ≡ 0 (l divides h) or h ≡ (l - 1) / 2 (l divides 2h + 1) modulo l.  The geometry, the tables
 *   and the workspace are those of mx_sieve (mx_safe_sieve_workspace_bytes = mx_sieve_workspace_bytes); limbs, table rows
 *   and multiply-adds are read and issued once for the two conditions.  Primes must be odd, >= 3 and < 2^31; limbs <= 1024.
 *   Two launches (the tables, the sieve) behind the upload of the list, no synchronisation.
 * mx_safe_double: d_out = 2 d_in + 1 over `rows` DEVICE rows [rows][limbs] (d_out must not be d_in); one launch.  A row
 *   whose top bit (bit 32 * limbs - 1) is set does not fit and comes out truncated: the caller refuses it beforehand.
 * A count of 0 returns MX_OK without a launch.  MX_ERR_ARG for a null pointer, limbs < 1, n_primes < 1, a negative count,
 * a listed prime that is even, below 3 or >= 2^31, or d_out == d_in; MX_ERR_SIZE for limbs > 1024 (the sieve) or more rows
 * than a launch addresses; MX_ERR_WORKSPACE for a workspace below mx_safe_sieve_workspace_bytes.  A refused call launches
 * nothing. */
int64_t mx_safe_sieve_workspace_bytes(int limbs, int n_primes);
int mx_safe_sieve(const uint32_t* d_halves, uint8_t* d_out, const uint32_t* h_primes, int n_primes, int limbs,
                  int64_t batch, void* d_workspace, int64_t workspace_bytes, void* stream);
int mx_safe_double(const uint32_t* d_in, uint32_t* d_out, int limbs, int64_t rows, void* stream);

/* ---- decryption proofs of a dealt threshold key: challenge and response (ABI 4.4, additions) -------------------------
 * The two steps of a proof of equal discrete logarithms that no other entry point covers (csrc/mx_sha256.hpp,
 * csrc/mx_response.hpp; tools/proof_model.py is the model; protocols/distributed_keygen_amd/threshold.py composes them with
 * the modexps, the multi-exponentiation and the fixed-base tables above).
 *
 * mx_sha256_rows:  d_out[r] = SHA-256(prefix | BE(rows_0[r]) | .. | BE(rows_{n_sets-1}[r])),  r < count  (FIPS 180-4).
 *   prefix: 32 HOST bytes that travel by value in the kernel-argument block (they may be freed or overwritten on return).
 *   d_rows: a HOST array of n_sets DEVICE pointers, set s being [count][limbs[s]] little-endian words; limbs: a HOST array.
 *   BE(row) is the row as a big-endian integer of 4 * limbs[s] bytes (its words in reverse order: they are the hash's
 *   big-endian message words, no byte is swapped), so the message has 32 + 4 * sum limbs bytes.  n_sets = 0 hashes the
 *   prefix alone, count times.  d_out is [count][8] little-endian words whose integer is the digest read as a big-endian
 *   integer (word 7 holds the digest's first four bytes).  One launch on `stream`, no workspace, no synchronisation.
 * mx_dleq_response:  d_z[r] = d_rho[r] + d_e[r] * x  over the integers,  r < count.
 *   d_rho [count][wz], d_e [count][ew], d_x ONE row [wx] (the secret exponent, resident on the device), d_z [count][wz]
 *   (it may be d_rho), d_status [count]: 1 iff the sum does not fit wz words (d_z[r] then holds its low wz words), else 0.
 *   Plain multiply-adds with carries, one row per lane; control flow and addresses depend on (count, wz, ew, wx) only.
 *   One launch on `stream`, no workspace, no synchronisation.
 * A count of 0 returns MX_OK without a launch.  MX_ERR_ARG for a null pointer (d_rows and limbs may be NULL when n_sets is
 * 0), n_sets outside [0, MX_SHA256_MAX_SETS], a width below 1 or a negative count; MX_ERR_SIZE for a message of more than
 * MX_SHA256_MAX_WORDS words, a width above MX_DLEQ_MAX_WORDS or more rows than a launch addresses.  A refused call
 * launches nothing. */
#define MX_SHA256_MAX_SETS 8
#define MX_SHA256_MAX_WORDS (1 << 24)
#define MX_DLEQ_MAX_WORDS (1 << 20)
int mx_sha256_rows(const uint8_t prefix[32], const uint32_t* const* d_rows, const int* limbs, int n_sets, int64_t count,
                   uint32_t* d_out, void* stream);
int mx_dleq_response(const uint32_t* d_rho, const uint32_t* d_e, const uint32_t* d_x, uint32_t* d_z, uint8_t* d_status,
                     int wz, int ew, int wx, int64_t count, void* stream);

/* ---- range proofs: multi-exponentiation over a generic odd modulus, per-row responses (ABI 4.4, additions) -----------
 * csrc/mx_multiexp.hpp, csrc/mx_response.hpp; tools/range_model.py is the model of the proofs that
 * protocols/distributed_keygen_amd/range_proof.py composes from them.
 *
 * mx_multiexp_run:  d_out[r] = prod_{t < terms} d_inputs[d_index[r][t]] ^ d_weights[r][t]  mod M,  r < n_outputs.
 *   h_mod: the odd modulus M >= 3, `limbs` HOST words (free on return).  d_inputs [n_inputs][limbs] residues below M,
 *   d_index int32 [n_outputs][terms] in [0, n_inputs) (an index outside it is clamped, never followed), d_weights
 *   [n_outputs][terms][ceil(weight_bits / 32)] little-endian words of NON-NEGATIVE weights, d_out [n_outputs][limbs]
 *   canonical residues in [0, M).  weight_bits, 1 .. MX_MULTIEXP_MAX_WEIGHT_BITS, is NOT tied to bits(M); bits of a
 *   weight at and above weight_bits, where the last word holds any, are read as part of the top window and must be 0.
 *   h_term_bits: NULL, or a HOST array of `terms` lengths in 0 .. weight_bits — the weights of term t are below
 *   2^h_term_bits[t] in EVERY row, and the windows above that length skip the term (a property of the launch, so control
 *   flow stays the same for every row); the entry of term 0 is prefetched, so the longest term goes first.
 *   0^0 = 1.  window 1 .. 8 (mx_multiexp_shape proposes one).  Interleaved fixed-window (Straus) form: a table pass (one
 *   group of lanes per input) and a main pass (one group per output) on `stream`, no synchronisation; control flow is
 *   the same for every row, only table addresses depend on the weights.  The workspace holds M, R mod M, the term lengths and the tables.
 * mx_multiexp_shape: lanes per element and limbs per lane of the instance that serves a modulus of mod_bits bits, and
 *   the window (the caller's when window > 0, else the one with the fewest Montgomery products whose tables stay within
 *   1 GiB).  mx_multiexp_workspace_bytes: bytes mx_multiexp_run needs for rows of `limbs` words and `terms` terms.
 * mx_multiexp_instances: the selectable (lanes, limbs per lane) pairs; returns their number and fills at most
 *   max_entries of them.
 * mx_response_rows:  d_z[r] = d_rho[r] + d_e[r] * d_x[r]  over the integers,  r < count: mx_dleq_response with a secret
 *   row PER PROOF, d_x [count][wx]; everything else — widths, status byte, data-independent control flow and addresses —
 *   as there.  A count of 0 returns MX_OK without a launch.
 * MX_ERR_ARG for a null pointer, limbs, n_inputs, n_outputs or terms below 1 (or above MX_MULTIEXP_MAX_TERMS, 2^31 - 1
 * rows), weight_bits outside 1 .. MX_MULTIEXP_MAX_WEIGHT_BITS, a term length outside 0 .. weight_bits, a window outside
 * 1 .. 8 (0 .. 8 for the shape query) — the shape and the workspace query refuse the same counts as the run —;
 * MX_ERR_MODULUS for an even modulus or one below 3; MX_ERR_SIZE for a modulus beyond the engine's widest;
 * MX_ERR_WORKSPACE.  A refused call launches nothing. */
#define MX_MULTIEXP_MAX_WEIGHT_BITS 16384
#define MX_MULTIEXP_MAX_TERMS 65536
int mx_multiexp_instances(int* lanes, int* limbs_per_lane, int max_entries);
int mx_multiexp_shape(int mod_bits, int64_t n_inputs, int64_t n_outputs, int terms, int weight_bits, int window,
                      int* lanes, int* limbs_per_lane_out, int* window_out);
int64_t mx_multiexp_workspace_bytes(int mod_bits, int limbs, int64_t n_inputs, int terms, int window);
int mx_multiexp_run(const uint32_t* h_mod, int limbs, const uint32_t* d_inputs, int64_t n_inputs, const int32_t* d_index,
                    const uint32_t* d_weights, int terms, int weight_bits, const int32_t* h_term_bits, uint32_t* d_out,
                    int64_t n_outputs, int window, void* d_workspace, int64_t workspace_bytes, void* stream);
int mx_response_rows(const uint32_t* d_rho, const uint32_t* d_e, const uint32_t* d_x, uint32_t* d_z, uint8_t* d_status,
                     int wz, int ew, int wx, int64_t count, void* stream);

/* ---- one-of-k membership proofs: the challenge arithmetic of the OR-composition (ABI 4.4, addition) ------------------
 * The one step of a Cramer-Damgard-Schoenmakers proof that c encrypts one of k public values which no other entry point
 * covers (csrc/mx_member.hpp; tools/member_model.py is the model; protocols/distributed_keygen_amd/membership.py composes
 * it with the modexps, the multi-exponentiation, the hash and the inverse above).  Rows of four little-endian words:
 * d_e [count][4] the challenges, d_sim and d_out [count][k][4] the per-branch challenges, d_index [count] the REAL branch
 * of each row (the prover's secret, in [0, k): an index outside it selects no branch), d_status [count].
 *   mode MX_MEMBER_MASK   d_out[r][j] = (j == d_index[r]) ? 0 : d_sim[r][j]
 *   mode MX_MEMBER_SPLIT  d_out[r][d_index[r]] = d_e[r] - sum_(j != d_index[r]) d_sim[r][j]  mod 2^128, the other slots copied
 *   mode MX_MEMBER_SUM    d_status[r] = (sum_j d_sim[r][j] mod 2^128 != d_e[r]); d_index and d_out are not read
 * One row per lane; control flow and addresses depend on (k, count) only — the real slot is selected by compare-and-mask
 * arithmetic, every slot of every row is read and written —, carries and borrows are add-with-compare.  d_out may be
 * d_sim.  A pointer a mode does not use (d_e for the mask; d_status for mask and split; d_index and d_out for the sum)
 * may be NULL.  One launch on `stream`, no workspace, no synchronisation; a count of 0 returns MX_OK without a launch.
 * MX_ERR_ARG for a null pointer the mode uses, k outside MX_MEMBER_MIN_K .. MX_MEMBER_MAX_K, a negative count or an
 * unknown mode; MX_ERR_SIZE for more rows than a launch addresses.  A refused call launches nothing. */
#define MX_MEMBER_MASK 0
#define MX_MEMBER_SPLIT 1
#define MX_MEMBER_SUM 2
#define MX_MEMBER_MIN_K 2
#define MX_MEMBER_MAX_K 16
int mx_member_challenges(const uint32_t* d_e, const uint32_t* d_sim, const int32_t* d_index, uint32_t* d_out,
                         uint8_t* d_status, int k, int64_t count, int mode, void* stream);

/* ---- multiplication proofs: the response modulo M with its quotient (ABI 4.4, addition) --------------------------------
 * The one step of a proof of correct multiplication (Damgard-Jurik 2001, section 4) which no other entry point covers
 * (csrc/mx_response_mod.hpp; tools/mul_model.py is the model; protocols/distributed_keygen_amd/multiplication.py composes
 * it with the modexps, the multi-exponentiation and the hash above): per row r < count
 *   s = d_rho[r] + d_e[r] * d_x[r] over the integers,   d_w[r] = s mod M,   d_t[r] = floor(s / M).
 * Little-endian words: d_rho, d_x and d_w [count][wn], d_e and d_t [count][ew], d_mod ONE modulus of wn words ON THE
 * DEVICE whose top word is non-zero (any such M, odd or even), d_status [count]: 1 iff the quotient does not fit ew words —
 * which happens only when d_rho[r] or d_x[r] is not below M —, d_t[r] then holds its low ew words and d_w[r] is the
 * correct residue all the same.  The two constants are the caller's, from M:
 *   shift = the number of leading zero bits of M's top word (0 .. 31),
 *   recip = floor(2^96 / (Md + 1)),  Md = the top 64 bits of M << shift (a one-word M: (M << shift) << 32),
 * so that 2^32 <= recip < 2^33; with other constants the rows are wrong, nothing else happens.
 * One row per lane; control flow and addresses depend on (wn, ew, count) only — quotient digits are estimated from the
 * top words and corrected by two masked subtractions, carries and borrows are add-with-compare —, no private segment, no
 * LDS.  d_w and d_t serve as the kernel's temporaries: NO OUTPUT MAY OVERLAP AN INPUT OR THE OTHER OUTPUT.  One launch on
 * `stream`, no workspace, no synchronisation; a count of 0 returns MX_OK without a launch.
 * MX_ERR_ARG for a null pointer, a width below 1, a negative count, a shift outside 0 .. 31 or a recip outside
 * [2^32, 2^33); MX_ERR_SIZE for a width above MX_DLEQ_MAX_WORDS or more rows than a launch addresses.  A refused call
 * launches nothing. */
int mx_response_mod_rows(const uint32_t* d_rho, const uint32_t* d_e, const uint32_t* d_x, const uint32_t* d_mod,
                         uint64_t recip, int shift, uint32_t* d_w, uint32_t* d_t, uint8_t* d_status, int wn, int ew,
                         int64_t count, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MXPAILLIER_H */
