/* C ABI of libntt.so — the MI355X-native drop-in for the reference's NTT host entry points.
 *
 * The reference (tie-pilot-qxw/NTT) has no library API: its entry points are C++ host drivers called
 * from main().  Each function below names the reference interface it replaces.
 *
 *   SSIP(long long* x, long long omega, uint log_n)            GZKP-NTT.cu:1452 (= self-sort-in-place.cu:309)
 *   NTT_GZKP<TPI,BITS>(cgbn_mem_t<bits> data[], uint len, uint2 reverse[], uint reverse_len,
 *                      cgbn_mem_t<bits> prime, cgbn_mem_t<bits> omega, uint B, uint G)
 *                                                               big-num.cu:260-261
 *   NTT_GZKP(long long data[], longlong2 reverse[], long long len, long long omega, int B, int G,
 *            long long reverse_num)                             parallel-load.cu:195 / GZKP-NTT.cu:167
 *   inverse: NTT(..., inv(root)) then * inv(len)               GZKP-NTT.cu:1725-1732 (commented out)
 *
 * Conventions (same as the reference unless stated):
 *   - data is a DEVICE pointer owned by the caller; transforms are in place, natural order in and
 *     out (the reference's SSIP contract), elements canonical (< p), not in Montgomery form;
 *   - element layout = cgbn_mem_t<32*W>: W little-endian 32-bit words (cgbn_cuda.h:51-55), i.e.
 *     limbs64 little-endian 64-bit limbs; the 1-limb P469762049 path uses `long long` elements;
 *   - `omega` arguments are the multiplicative GENERATOR (the reference passes `root`, 3), the
 *     n-th root is omega^((p-1)/n) (GZKP-NTT.cu:1462, big-num.cu:292-296);
 *   - unlike the reference (void, prints timings, default stream, blocking): every call returns a
 *     status (0 ok, < 0 error, see ntt_strerror), prints nothing, and the plan API is asynchronous
 *     on the given hipStream_t (NULL = default stream).  The reference-shaped shims SSIP /
 *     NTT_GZKP_256 keep the reference's blocking behaviour.
 *   - plans are thread-compatible: one plan per thread, or serialise calls on a plan.  A plan's
 *     scratch is shared by its calls, so calls on one plan must also be ordered on the device (the
 *     same stream, or streams the caller orders).  The status of the last call (ntt_last_error) is
 *     kept per thread.  The shims are thread-safe: their plan cache is locked and each cached plan
 *     runs one blocking call at a time.
 */
#ifndef NTT_AMD_NTT_H
#define NTT_AMD_NTT_H
#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

/* status codes */
#define NTT_OK 0
#define NTT_ERR_ARG (-1)      /* invalid field / size / limb count / pointer */
#define NTT_ERR_HIP (-2)      /* HIP runtime error (launch, allocation, copy) */
#define NTT_ERR_RCCL (-3)     /* RCCL error (multi-GPU) */
#define NTT_ERR_FIELD (-4)    /* modulus unsupported (even, too large, no root of unity of order n) */
#define NTT_ERR_NODEV (-5)    /* no HIP device */
#define NTT_ERR_DEVICE (-6)   /* an inter-workgroup wait of an earlier call on this plan gave up at its
                               * watchdog (in-place or single-launch schedules; never expected): that
                               * call's output is wrong.  Every call on the plan returns this until
                               * ntt_plan_device_status clears the report.  The blocking shims return it
                               * for the call itself (and clear it).  The reference asserts instead
                               * (GZKP-NTT.cu:1527). */

/* field ids */
#define NTT_FIELD_P469762049 0   /* 7*2^26+1, generator 3 (GZKP-NTT.cu:7-8) */
#define NTT_FIELD_BN254_FR 1     /* 0x30644e72...f0000001, generator 5 */
#define NTT_FIELD_BLS12_381_FR 2 /* 0x73eda753...00000001, generator 7 */
#define NTT_FIELD_GOLDILOCKS 3   /* 2^64 - 2^32 + 1 = 0xffffffff00000001, generator 7, two-adicity 32;
                                  * 1 limb: 8-byte uint64_t elements */
#define NTT_FIELD_BABYBEAR 4     /* 2^31 - 2^27 + 1 = 0x78000001, generator 31, two-adicity 27;
                                  * 1 limb: 4-byte uint32_t elements */
#define NTT_FIELD_KOALABEAR 5    /* 2^31 - 2^24 + 1 = 0x7f000001, generator 3, two-adicity 24;
                                  * 1 limb: 4-byte uint32_t elements */

typedef struct ntt_plan ntt_plan;

/* Create a plan for 2^log_n-point transforms on `device` (twiddle tables and scratch are cached in
 * the plan: the reference rebuilt its tables on every call, GZKP-NTT.cu:1476-1500).
 * limbs64: 1 (P469762049, `long long` elements, and Goldilocks, `uint64_t` elements; Goldilocks takes
 * no other limb count), 4 (256-bit, cgbn_mem_t<256>), 6 (384-bit template).  Replaces the table setup
 * inside SSIP (GZKP-NTT.cu:1452-1505) and NTT_GZKP (big-num.cu:278-309).
 * Goldilocks plans (the built-in field, or a custom 1-limb plan of that modulus) run every call of
 * this header on canonical 8-byte elements, log_n 0..32.  Of the flags below they take
 * NTT_PLAN_TWIDDLE_ONLY and ignore NTT_PLAN_SINGLE_LAUNCH; NTT_PLAN_MONTGOMERY_IO, NTT_PLAN_IN_PLACE
 * and the rival schedules return NTT_ERR_ARG.
 * BabyBear and KoalaBear plans (and NTT_PLAN_ELEM32 custom plans) run every call of this header on
 * canonical 4-byte uint32_t elements, limbs64 = 1 only (any other count: NTT_ERR_ARG), log_n up to the
 * field's two-adicity (27 / 24; above it NTT_ERR_FIELD); ntt_plan_info reports elem_bytes 4.  A coset
 * shift is still one uint64_t holding a value below p.  They take NTT_PLAN_TWIDDLE_ONLY and
 * NTT_PLAN_MONTGOMERY_IO (with R = 2^32), ignore NTT_PLAN_SINGLE_LAUNCH, and return NTT_ERR_ARG for
 * NTT_PLAN_IN_PLACE and the rival schedules.  ntt_rplan_create accepts them; ntt_mplan_create returns
 * NTT_ERR_ARG (its exchange sizes count 8-byte words). */
int ntt_plan_create(ntt_plan** out, int field_id, unsigned log_n, unsigned limbs64, int device);

/* Plan flags for the _ex constructors. */
#define NTT_PLAN_TWIDDLE_ONLY 1u /* only the w_n tables: fill / twiddle_pack / transpose, no transforms */
/* Elements are in Montgomery form x R mod p, R = 2^(64 limbs64) -- R = 2^32 on the 4-byte elements of
 * NTT_PLAN_ELEM32 plans, the form Plonky3 and RISC Zero keep BabyBear in -- (CGBN's bn2mont domain,
 * impl_cuda.cu:980-1010; the form arkworks / sppark / ICICLE callers keep their data in).  The
 * transforms are linear, so forward / inverse / coset are unchanged (NTT(x R) = NTT(x) R); the
 * pointwise product becomes the Montgomery product a b R^-1 so that polymul maps (a R, b R) to
 * (a b) R.  Saves the caller a to/from-Montgomery pass over the data on each side. */
#define NTT_PLAN_MONTGOMERY_IO 2u
/* Rival schedule: forward transforms run as the reference's bellperson / improved_NTT
 * family re-derived for gfx950 — Stockham autosort passes of radix 2^r_i with the twiddle applied to
 * the INPUT of each pass (GZKP-NTT.cu:324-386 FIELD_radix_fft; :556-1296 improved_NTT_v1..v4, whose
 * grouping / coalescing / bank-conflict variants the wave64 LDS-staged kernels subsume), ping-pong
 * between two plan buffers, no final digit-reversal pass.  Same contract and results as the default
 * four-step DIF schedule; kept to measure against it (tools/bench_rivals.py).  P469762049 (1 limb)
 * and 4-limb plans, single transforms (batch 1); other calls use the default schedule. */
#define NTT_PLAN_STOCKHAM 4u
/* Rival schedule: forward transforms run as the reference's GZKP(B, G) (GZKP-NTT.cu:
 * 115-165, driver 167-233; parallel-load.cu:114-193 for P): a bit-reversal permutation pass
 * (`rearrange`), then in-place radix-2 DIT rounds, B of them per pass over tiles of G adjacent
 * columns, re-derived as: the permutation into a plan buffer, a first pass of contiguous radix-2^r_0
 * DFTs, then passes that multiply their inputs by w_N^(c d) (per-pass tables) and run radix-2^r_i
 * DFTs in place over stride-2^(r_0 + .. + r_{i-1}) columns.  Same contract and results as the
 * default schedule; P469762049 (1 limb) and 4-limb plans, single transforms (batch 1).
 * NTT_PLAN_STOCKHAM and NTT_PLAN_GZKP are exclusive. */
#define NTT_PLAN_GZKP 8u
/* In place, no scratch (the reference's self-sort-in-place property, SSIP_NTT_stage2's mirror pairs,
 * GZKP-NTT.cu:1359-1449): the plan owns no n-element buffer.  The radices are arranged as a
 * palindrome (R_1 = R_p, middle radices symmetric; one pass more than the default schedule when
 * log_n admits no palindrome of that length, e.g. odd log_n over an even pass count), every pass
 * writes the positions it read, and the digit reversal (an involution) is fused into the final
 * pass: each final tile writes natural positions once the mirror slab has been read (k_final_ipn,
 * bounded waits reported by ntt_plan_device_status); batched calls take a separate pass of disjoint
 * tile-pair swaps instead.  Same contract and results as the default schedule, within ~1 % of its
 * time on the 256-bit path.  P469762049 plans run on 8-B scratch elements for it (the default P
 * plan keeps 4-B ones); 6 x 64-bit plans of a modulus < 2^255 keep their intermediates in the
 * caller's 48-B elements (the default 6-limb plan uses 32-B scratch).  Sizes with no palindrome the
 * pass kernels accept (2^11 and 2^13 on the 1024-element tiles; P: 2^15, 2^17, 2^19 on its
 * 8192-element tiles) and the rival schedules return NTT_ERR_ARG. */
#define NTT_PLAN_IN_PLACE 16u
/* Single-launch schedule (BASELINE config 2, "single-kernel self-sort-in-place"; the reference runs
 * 2^20 as 4 launches, GZKP-NTT.cu:1509-1545): a forward / inverse of a 4-limb BN254 / BLS12-381 plan
 * runs as ONE persistent launch.  At 2^20 (round 5): the two passes of 4096-element tiles (10 + 10)
 * with one grid barrier (k_fused2b); with NTT_PLAN_IN_PLACE too, no scratch and a second barrier
 * before the digit-reversed stores (k_fused2bi).  Other 3-pass sizes (2^18 .. 2^24): two grid-wide
 * barriers (k_fused3b; the default) or the passes' tiles handed between workgroups through dependency
 * counters (k_fused3; environment NTT_FUSED_MODE=0); in place (2^18, 2^19): three barriers
 * (k_fused3bi).  Same contract and results as the default schedule; batch 1; other plans and calls
 * ignore the flag.
 * The grid-barrier forms are plain launches of at most as many workgroups as the device keeps
 * resident (the plan's occupancy query).  The library orders them per device (round 6): a single
 * launch enqueued on another stream than the device's previous one waits for it, so two
 * single-launch plans on two streams never split the device between them (on one stream nothing is
 * added).  CUs held by anything else (another process, a persistent kernel of the caller's) can still
 * keep part of a launch waiting; every wait is bounded, so the call then returns garbage and the
 * plan's next call NTT_ERR_DEVICE (ntt_plan_device_status), never a hang.  The in-place forms
 * (k_fused2bi, k_fused3bi) check residency before their first store: such a call stores nothing and
 * the caller's buffer keeps its input.  (The cooperative-launch switch NTT_FUSED_COOP was retired in
 * round 6.)
 * ntt_plan_device_status reports a wait that gave up (a watchdog; never expected). */
#define NTT_PLAN_SINGLE_LAUNCH 32u
/* Rival schedule, the reference's `naive` (GZKP-NTT.cu:59-95, big-num.cu:67-170): the bit reversal,
 * then log2 n radix-2 DIT rounds of one launch each (a thread per butterfly, w from an n/2-entry power
 * table, the reference's `roots`).  Forward single transforms of P469762049 and 4-limb plans; the
 * plan's other calls run the default schedule.  Exclusive with the other rivals and with
 * NTT_PLAN_IN_PLACE. */
#define NTT_PLAN_NAIVE 64u
/* Rival schedule, the reference's `naive_no_swap` (GZKP-NTT.cu:237-296; its main checks it against
 * the CPU NTT, GZKP-NTT.cu:1653-1660): a radix-2 Stockham autosort -- log2 n rounds of one launch
 * each, round s reading x[i], x[i + n/2] and writing y[2i - k], y[2i - k + 2^s] (k = i mod 2^s,
 * w = w_n^(k n / 2^(s+1)) from the n/2-entry power table), ping-pong between the caller's buffer and
 * a plan buffer, natural order in and out, no bit reversal.  When log2 n is odd the last round lands
 * in the plan buffer and one device copy brings it back.  Forward single transforms of P469762049 and
 * 4-limb plans; the plan's other calls run the default schedule.  Exclusive with the other rivals and
 * with NTT_PLAN_IN_PLACE. */
#define NTT_PLAN_NO_SWAP 128u
/* Rival schedules, the reference's bealto.com radix-2^deg Stockham family (round 6): log2 n / deg
 * rounds of one launch each, ping-pong between the caller's buffer and a plan buffer, natural order
 * in and out.  A group of 2^deg elements x[index + i t] (t = n / 2^deg) is multiplied by
 * w^((n >> lgp >> deg) k i) (k = index mod 2^lgp), transformed by deg radix-2 rounds in LDS with the
 * 2^(max_deg-1)-entry table pq, and written to y[((index - k) << deg) + k + i 2^lgp]; two elements per
 * thread.  The variants differ only in how threads, groups and LDS rows map (the reference's access
 * patterns, kept for comparison):
 *   NTT_PLAN_BELLPERSON   bellperson_baseline / FIELD_radix_fft_revised (GZKP-NTT.cu:391-553): one
 *                         group per workgroup, deg <= 8, inputs bit-reversed into LDS, DIT rounds;
 *   NTT_PLAN_IMPROVED_V1  improve_grouped (GZKP-NTT.cu:556-630, 721-804): 32 groups per workgroup,
 *                         deg <= 3, DIF rounds, outputs bit-reversed from LDS;
 *   NTT_PLAN_IMPROVED_V2  improve_group_coalesced_read (632-719, 806-890): v1 with the load map
 *                         transposed, consecutive threads reading consecutive groups;
 *   NTT_PLAN_IMPROVED_V3  improve_group_coalesced_read_and_write (892-1075): v2 with the stores on
 *                         the load map too (after the first round);
 *   NTT_PLAN_IMPROVED_V4  improve_reduce_bank_conflict (1077-1296): v3 with each group's LDS row
 *                         padded by one element.
 * The reference runs them on P469762049 (`long long`); here forward single transforms of P469762049
 * and 4-limb plans, the plan's other calls on the default schedule.  Exclusive with the other rivals
 * and with NTT_PLAN_IN_PLACE. */
#define NTT_PLAN_BELLPERSON 256u
#define NTT_PLAN_IMPROVED_V1 512u
#define NTT_PLAN_IMPROVED_V2 1024u
#define NTT_PLAN_IMPROVED_V3 2048u
#define NTT_PLAN_IMPROVED_V4 4096u
/* 4-byte elements: with ntt_plan_create_custom_ex and limbs64 = 1, a plan for any odd prime p < 2^31
 * with 2^log_n | p - 1 on canonical uint32_t elements (the 31-bit engine: values canonical between all
 * operations, so p may exceed 2^30).  Any other limb count returns NTT_ERR_ARG, a modulus >= 2^31
 * (Goldilocks included) NTT_ERR_FIELD.  Implied (and accepted) on NTT_FIELD_BABYBEAR and
 * NTT_FIELD_KOALABEAR; NTT_ERR_ARG on fields 0-3.  Without the flag nothing changes: a 1-limb custom
 * plan of a modulus >= 2^30 other than Goldilocks still returns NTT_ERR_FIELD. */
#define NTT_PLAN_ELEM32 8192u
int ntt_plan_create_ex(ntt_plan** out, int field_id, unsigned log_n, unsigned limbs64, int device, unsigned flags);
/* Device-side status of a plan (blocking: synchronises the device, then reads and clears it).
 * *bad bit 0: an inter-workgroup wait gave up at its watchdog (NTT_PLAN_SINGLE_LAUNCH, or the fused
 * digit reversal of NTT_PLAN_IN_PLACE): that call's output is wrong (the workgroup that gave up
 * skipped its stores), and until this call clears the report every other call on the plan returns
 * NTT_ERR_DEVICE.  The checked build (ntt_amd/libntt_debug.so,
 * same ABI, `python -m ntt_amd.build --debug`) adds, from checks inside every pass kernel:
 *   0x100  an element index outside its buffer (the access went to element 0 instead)
 *   0x200  a caller input element >= p (the inputs must be canonical, as in the reference)
 *   0x400  an intermediate >= 2p (a lazy-reduction bound broke; Goldilocks and 4-byte-element plans
 *          keep no lazy values: an intermediate >= p)
 *   0x800  an output element >= p
 * The product build never sets these bits. */
int ntt_plan_device_status(ntt_plan* plan, unsigned* bad);
/* Poll limit of the plan's bounded inter-workgroup waits (default 2^21, about 2 s; read at each
 * launch).  0 makes every wait that is not already satisfied give up at once: a test hook for the
 * NTT_ERR_DEVICE path (tests/test_gpu_watchdog.py). */
int ntt_plan_set_watchdog(ntt_plan* plan, unsigned spins);

/* Modulus-generic plan, like big-num.cu's `prime` / `omega` kernel arguments (big-num.cu:68,173,260):
 * modulus and generator given as limbs64 little-endian 64-bit limbs.  Accepted moduli: odd primes
 * with 2^log_n | p - 1 and, by limb count, p < 2^30 or exactly the Goldilocks prime 0xffffffff00000001
 * on 8-byte uint64_t elements (1 limb: lazy values up to 4p must fit 32 bits, so every other modulus
 * >= 2^30, e.g. the 31-bit 2013265921, returns NTT_ERR_FIELD; with NTT_PLAN_ELEM32 any p < 2^31 on
 * 4-byte uint32_t elements), p < 2^255 (4 limbs), p < 2^(29*14-6) with 2p below 2^383 (6 limbs). */
int ntt_plan_create_custom(ntt_plan** out, const uint64_t* modulus, const uint64_t* generator, unsigned limbs64,
                           unsigned log_n, int device);

int ntt_plan_create_custom_ex(ntt_plan** out, const uint64_t* modulus, const uint64_t* generator, unsigned limbs64,
                              unsigned log_n, int device, unsigned flags);

/* Forward NTT in place, natural -> natural (SSIP GZKP-NTT.cu:1452, NTT_GZKP big-num.cu:260). */
int ntt_forward(ntt_plan* plan, void* d_data, void* hip_stream);
/* Inverse NTT in place including the n^-1 scale (GZKP-NTT.cu:1725-1732). */
int ntt_inverse(ntt_plan* plan, void* d_data, void* hip_stream);
/* `batch` independent transforms laid out back to back (stride 2^log_n elements). */
int ntt_forward_batch(ntt_plan* plan, void* d_data, unsigned batch, void* hip_stream);
int ntt_inverse_batch(ntt_plan* plan, void* d_data, unsigned batch, void* hip_stream);

/* Coset NTT of one vector of the plan's own size, in place:
 *   forward:  X_k = sum_j x_j (c w^k)^j = NTT(x_j c^j)          (evaluations on the coset c<w>)
 *   inverse:  x_j = c^-j INTT(X)_j                               (interpolation from the coset)
 * `shift` = c as limbs64 little-endian 64-bit limbs, canonical and nonzero (e.g. the field's
 * multiplicative generator).  The plan caches the c^j tables of the last shift.  This is not a
 * low-degree extension: it neither pads nor batches (ntt_lde_batch below does). */
int ntt_forward_coset(ntt_plan* plan, void* d_data, const uint64_t* shift, void* hip_stream);
int ntt_inverse_coset(ntt_plan* plan, void* d_data, const uint64_t* shift, void* hip_stream);

/* Low-degree extension.  `plan` is a plan of the LARGE size N = 2^log_n.  d_in holds `batch`
 * polynomials back to back, n = 2^(log_n - log_blowup) coefficients each (stride n elements);
 * d_out receives `batch` vectors of N evaluations each (stride N elements), natural order:
 *     out[v][k] = sum_{j < n} in[v][j] (c w_N^k)^j ,   c = *shift, or 1 when shift == NULL.
 * d_in is not modified.  Asynchronous on hip_stream.
 * 0 <= log_blowup <= log_n: 0 is an out-of-place batched coset forward, log_n extends constants.
 * `shift` follows ntt_forward_coset (canonical, nonzero, limbs64 words; canonical also on
 * NTT_PLAN_MONTGOMERY_IO plans, whose data stay in Montgomery form) and shares its cached tables
 * (except on 4-limb plans of 2^20, where ntt_forward_coset runs on the plan's 4096-element tiles
 * with a cache of its own); a call with shift == NULL leaves the cached shift as it is.
 * The zero padding is never written or read: the first pass loads the n coefficients of each
 * polynomial, multiplied by c^j at that load (6-limb moduli above 2^255 and plans without the fast
 * reductions: by one launch over the batch n inputs before it), and takes every other input from
 * registers.  Sizes up to 4 points, and a few custom-modulus plans whose first pass has no such form
 * (DESIGN.md section 4), stage the zero-padded vectors in d_out instead.
 * NTT_ERR_ARG before any launch: a null plan or pointer, batch == 0, log_blowup > log_n, a bad
 * shift, overlapping byte ranges of d_in (batch n elements) and d_out (batch N elements),
 * NTT_PLAN_TWIDDLE_ONLY and NTT_PLAN_IN_PLACE plans.  Rival-schedule and NTT_PLAN_SINGLE_LAUNCH
 * plans run it on the default schedule; 4-limb plans of 2^20 on their 1024-element tiles. */
int ntt_lde_batch(ntt_plan* plan, const void* d_in, void* d_out, unsigned log_blowup, const uint64_t* shift,
                  unsigned batch, void* hip_stream);

/* Transforms over the COLUMNS of a row-major matrix: 2^log_n rows of `width` elements, one polynomial
 * per column, element (j, b) at d_data[j * width + b] (j < 2^log_n, b < width) -- the layout a STARK
 * prover keeps a trace or a batch of committed polynomials in, each row of the result being one Merkle
 * leaf.  A vector over a degree-d extension field, stored as d adjacent base-field coefficients per
 * element and transformed with base-field twiddles, is such a matrix of d * width columns.  `width` is
 * any positive number with 2^log_n * width < 2^32; there is no row pitch other than `width`.
 *   ntt_forward_matrix / ntt_inverse_matrix: every column transformed in place as ntt_forward /
 *     ntt_inverse would (natural order, canonical elements, 1/n included in the inverse);
 *   ntt_lde_matrix: `plan` has the LARGE size N = 2^log_n; d_in is [n = N >> log_blowup][width],
 *     d_out [N][width], out[k][b] = sum_{j < n} in[j][b] (c w_N^k)^j, c = *shift, or 1 when shift == NULL.
 *     d_in is not modified.  `shift` and its cached tables as ntt_lde_batch.
 * Asynchronous on hip_stream.  With width == 1 the results are those of ntt_forward / ntt_inverse /
 * ntt_lde_batch(batch = 1) bit for bit.  NTT_PLAN_MONTGOMERY_IO plans keep their data in Montgomery form
 * (the transforms are linear); NTT_PLAN_SINGLE_LAUNCH is ignored.
 * The data are never transposed, padded or staged: every pass reads and writes the matrix (or a plan
 * scratch of exactly 2^log_n * width elements) once, a workgroup working on a strip of adjacent columns
 * (at least 64 bytes of every row it touches, the whole row when that is shorter); the zero rows of an
 * extension are never read or written.  The calls run a schedule of their own
 * (ntt_plan_matrix_info: its pass count, 0 for sizes up to 4 rows, and log2 radices at this width), whose
 * tables the plan builds at its first matrix call.
 * Engines: Goldilocks, BabyBear, KoalaBear and NTT_PLAN_ELEM32 custom plans, at every log_n the plan
 * accepts.  Plans of fields 0-2 and of custom 4- and 6-limb moduli return NTT_ERR_ARG from all four
 * calls for now.
 * NTT_ERR_ARG before any launch: a null plan or pointer, width == 0, 2^log_n * width >= 2^32,
 * log_blowup > log_n, a bad shift, overlapping byte ranges of d_in and d_out, NTT_PLAN_TWIDDLE_ONLY
 * plans. */
int ntt_forward_matrix(ntt_plan* plan, void* d_data, unsigned width, void* hip_stream);
int ntt_inverse_matrix(ntt_plan* plan, void* d_data, unsigned width, void* hip_stream);
int ntt_lde_matrix(ntt_plan* plan, const void* d_in, void* d_out, unsigned log_blowup, const uint64_t* shift,
                   unsigned width, void* hip_stream);
int ntt_plan_matrix_info(const ntt_plan* plan, unsigned width, unsigned* npasses, unsigned radix_log[8]);

/* The matrix calls on a coset and with the evaluations' rows in bit-reversed order: the two steps around
 * a prover's extension (quotient evaluations on c<w_n> back to coefficients; rows stored so that FRI's
 * fold partners k and k + N/2 are adjacent and the first N / 2^k rows are a sub-coset).
 *   ntt_forward_matrix_ex: in place, out[k][b] = sum_j in[j][b] (c w_n^k)^j -- the product by c^j rides at
 *     the first pass's load, as in ntt_lde_matrix;
 *   ntt_inverse_matrix_ex: in place, out[j][b] = c^-j INTT(column b)_j -- the product by c^-j rides at
 *     the last pass's store;
 *   ntt_lde_matrix_ex: ntt_lde_matrix with `order`.
 * c = *shift, canonical and nonzero (one uint64_t on these engines; canonical on NTT_PLAN_MONTGOMERY_IO
 * plans too), sharing ntt_lde_batch's cached tables; shift == NULL is c = 1: no product, and the shift
 * cache is not touched.
 * order: NTT_MATRIX_BITREV_OUT (forward, lde): row k of the natural result is stored at row
 * bitrev(k); NTT_MATRIX_BITREV_IN (inverse): row i of d_data holds the evaluation of natural index
 * bitrev(i).  bitrev reverses the plan's log_n bits (for an lde: of the large size N).  A row map picks
 * another row for the same run of columns, so it costs no coalescing; neither option adds a launch, a pass
 * or a buffer, and ntt_plan_matrix_info and the launch labels are those of the plain calls.
 * With shift == NULL and order == 0 each call is its plain form: the same launches, the same bits.
 * NTT_ERR_ARG before any launch, the buffers untouched: whatever the plain calls refuse, an unknown bit in
 * `order`, NTT_MATRIX_BITREV_IN on forward or lde, NTT_MATRIX_BITREV_OUT on inverse, a bad shift. */
#define NTT_MATRIX_BITREV_OUT 1u
#define NTT_MATRIX_BITREV_IN 2u
int ntt_forward_matrix_ex(ntt_plan* plan, void* d_data, unsigned width, const uint64_t* shift, unsigned order,
                          void* hip_stream);
int ntt_inverse_matrix_ex(ntt_plan* plan, void* d_data, unsigned width, const uint64_t* shift, unsigned order,
                          void* hip_stream);
int ntt_lde_matrix_ex(ntt_plan* plan, const void* d_in, void* d_out, unsigned log_blowup, const uint64_t* shift,
                      unsigned width, unsigned order, void* hip_stream);

/* FRI fold of bit-reversed coset evaluations: the step after ntt_lde_matrix_ex(..., width = d,
 * NTT_MATRIX_BITREV_OUT), which consumes the order that call stores.  An extension element is ext_degree = d
 * adjacent base-field coefficients, an element of the ring F_p[X]/(X^d - W), W = ext_w (the library does the
 * ring arithmetic and does not test irreducibility); d = 1 is the base field.
 * With L = log_rows, N = 2^L, k = log_arity, M = N >> k, c = *shift (1 when shift == NULL), w_N the plan's
 * root g^((p-1)/N) and rev_b the reversal of b bits:
 *   d_in  [N][d]: row i holds f(c w_N^rev_L(i)) for a polynomial f of degree < N with extension coefficients;
 *   d_out [M][d]: with f(x) = sum_{t < 2^k} x^t f_t(x^(2^k)) and g(y) = sum_t beta^t f_t(y), row i' holds
 *                 g(c^(2^k) w_M^rev_{L-k}(i')): the same convention one level down, on the coset
 *                 c^(2^k) <w_M>, so folds chain with c^(2^k) as the next shift.
 * In the evaluation domain: rows i' 2^k + j (j < 2^k) are the fibre over row i', at the points
 * x0 zeta^rev_k(j), x0 = c w_N^rev_{L-k}(i'), zeta = w_N^M; u_t = 2^-k sum_j zeta^(-t rev_k(j)) in[i' 2^k + j]
 * and out[i'] = sum_t (beta / x0)^t u_t -- for k = 1 the usual (lo + hi) / 2 + beta (lo - hi) / (2 x0).
 * One fold of arity 2^k by beta equals k folds of arity 2 by beta, beta^2, beta^4, ... with shifts c, c^2,
 * c^4, ..., bit for bit.
 * log_rows is any value from log_arity up to the plan's log_n (one plan of the largest layer serves every
 * later one); 1 <= log_arity <= 4; ext_degree 1, 2 or 4; ext_w canonical and nonzero when ext_degree > 1,
 * ignored at 1; beta: ext_degree host words, each canonical; shift: one canonical nonzero host word or NULL,
 * as ntt_forward_matrix_ex takes it -- but nothing is cached: the shift tables of the other calls are not
 * touched (c^-1 is one host inversion per call).  beta, ext_w and shift are canonical on
 * NTT_PLAN_MONTGOMERY_IO plans too; the data keep the plan's form: every product is by a constant or by a
 * per-row scalar t held as t R, and mulv(x, t R) = x t in whichever form x is, so one code path serves both
 * plan kinds and the outputs carry the inputs' form.
 * Asynchronous on hip_stream; one launch; d_in is not modified; outputs are canonical.
 * Engines: as the matrix calls (Goldilocks, BabyBear, KoalaBear, NTT_PLAN_ELEM32 custom plans); plans of
 * fields 0-2 and of custom 4- and 6-limb moduli return NTT_ERR_ARG.
 * NTT_ERR_ARG before any launch, the buffers untouched: a null plan or pointer, log_arity 0, above 4 or above
 * log_rows, log_rows above the plan's log_n, ext_degree outside {1, 2, 4}, ext_w 0 or >= p when
 * ext_degree > 1, a beta word >= p, a bad shift, overlapping byte ranges of d_in (N d elements) and d_out
 * (M d elements), NTT_PLAN_TWIDDLE_ONLY plans. */
int ntt_fri_fold(ntt_plan* plan, const void* d_in, void* d_out, unsigned log_rows, unsigned log_arity,
                 unsigned ext_degree, uint64_t ext_w, const uint64_t* beta, const uint64_t* shift,
                 void* hip_stream);

/* DEEP openings and quotients of a row-major coset evaluation matrix: what lies between
 * ntt_lde_matrix_ex(..., NTT_MATRIX_BITREV_OUT) and ntt_fri_fold.
 * With L = log_rows (0 <= L <= the plan's log_n), N = 2^L, w_N = w_n^(n/N) from the plan's root, c = *shift
 * (1 when NULL), sigma the identity when order == 0 and rev_L when order == NTT_MATRIX_BITREV_OUT, and
 * x_i = c w_N^sigma(i): M = d_mat = [N][width] holds base-field rows, column j the evaluations p_j(x_i) of a
 * polynomial of degree < N.  An extension element is d = ext_degree in {1, 2, 4} adjacent base coefficients of
 * F_p[X]/(X^d - W), W = ext_w, as in ntt_fri_fold.  M, d_values and d_out are in the plan's I/O form
 * (Montgomery on NTT_PLAN_MONTGOMERY_IO plans); the host words z, alpha, scale, ext_w and shift are always
 * canonical.
 *   ntt_deep_points  d_inv [N][d]: d_inv[i] = (z - x_i)^-1 in the WORKING FORM: on the 4-byte engines the value
 *     times 2^32 mod p, for every plan kind; on Goldilocks the plain value.  (A Montgomery product of such a
 *     value with a datum in either I/O form is the plain product in the datum's form; ntt_fri_fold holds its
 *     t R the same way.)  x_i comes from the plan's two-level tables at stride 2^(log_n - log_rows): no table
 *     is built.  Each thread inverts a run of 16 / d (4-byte engines; 8 / d on Goldilocks) consecutive rows with
 *     one extension inversion (Montgomery's batch trick).  NTT_ERR_ARG before any launch when z lies in the
 *     base field (d = 1, or coordinates 1.. all zero) and z_0^N = c^N: the only case in which z hits the
 *     domain.  Where X^d - W is reducible and some z - x_i is not invertible, the rows of that run are
 *     unspecified; nothing faults.
 *   ntt_matrix_open  d_values [width][d]: d_values[j] = p_j(z), by the barycentric form
 *     p_j(z) = (z^N - c^N) / (N c^N) sum_i M[i][j] x_i / (z - x_i), with x_i / (z - x_i) = z / (z - x_i) - 1: two
 *     sums over the rows, sum_i M[i][j] d_inv[i] and sum_i M[i][j].  d_inv is ntt_deep_points' output for the
 *     same log_rows, ext_degree, ext_w, z, shift and order.  Two launches: strips of columns x chunks of rows into
 *     a plan-owned buffer (allocated at the first use, its size independent of N), then the chunks in order
 *     and the two host-computed scalars.  No atomics: the same bits every run.  The base-field z of the coset
 *     is NTT_ERR_ARG here too.
 *   ntt_deep_quotient  d_out [N][d]:
 *       d_out[i] = scale d_inv[i] (sum_j alpha^j v_j - sum_j alpha^j M[i][j]),  v_j = d_values[j],
 *     which is scale sum_j alpha^j (p_j(x_i) - v_j) / (x_i - z).  scale == NULL is 1.  flags &
 *     NTT_DEEP_ACCUMULATE adds into d_out (its elements canonical in the plan's form), so several opening
 *     points or matrices sum into one codeword, with scale = alpha^width for the second.  The row order lives
 *     in d_inv.  Two launches: the table scale alpha^j (each entry by square and multiply) and
 *     V = scale sum_j alpha^j v_j into the plan-owned buffer, then the rows: 2^k lanes share a row and stride its
 *     columns, 2^k a quarter of the largest power of two up to the width, at least 64 bytes of lanes (16 on
 *     4-byte elements, 8 on 8-byte ones) and at most 64; rows shorter than 64 bytes take one lane per row, each
 *     lane several rows in turn and each wave reading 64 consecutive rows at a time.
 *   ntt_deep_info  the two shape decisions at (width, log_rows, ext_degree): the row chunks of ntt_matrix_open
 *     and the lanes per row of ntt_deep_quotient.  No launch.
 * The three launching calls are asynchronous on hip_stream and never synchronise the host.  Any
 * element-aligned pointer is accepted; 16-byte accesses are used when the pointers are 16-byte aligned.
 * Engines: as the matrix calls; plans of fields 0-2 and of custom 4- and 6-limb moduli return NTT_ERR_ARG.
 * NTT_ERR_ARG before any launch, the buffers untouched: a null plan or pointer (shift and scale may be NULL),
 * width 0, N width >= 2^32, log_rows above the plan's log_n, ext_degree outside {1, 2, 4}, ext_w 0 or >= p when
 * ext_degree > 1 (ignored at 1), a z, alpha, scale or shift word >= p, a zero shift, an unknown bit in order
 * or flags, NTT_PLAN_TWIDDLE_ONLY plans, overlapping byte ranges of an output with any input. */
#define NTT_DEEP_ACCUMULATE 1u
int ntt_deep_points(ntt_plan* plan, void* d_inv, unsigned log_rows, unsigned ext_degree, uint64_t ext_w,
                    const uint64_t* z, const uint64_t* shift, unsigned order, void* hip_stream);
int ntt_matrix_open(ntt_plan* plan, const void* d_mat, unsigned width, unsigned log_rows, const void* d_inv,
                    unsigned ext_degree, uint64_t ext_w, const uint64_t* z, const uint64_t* shift, unsigned order,
                    void* d_values, void* hip_stream);
int ntt_deep_quotient(ntt_plan* plan, const void* d_mat, unsigned width, unsigned log_rows, const void* d_inv,
                      const void* d_values, unsigned ext_degree, uint64_t ext_w, const uint64_t* alpha,
                      const uint64_t* scale, unsigned flags, void* d_out, void* hip_stream);
int ntt_deep_info(const ntt_plan* plan, unsigned width, unsigned log_rows, unsigned ext_degree,
                  unsigned* open_row_chunks, unsigned* quotient_lanes_per_row);

/* Poseidon2 Merkle commitments and openings of a row-major matrix: the step between ntt_lde_matrix_ex,
 * ntt_deep_quotient, ntt_fri_fold and the next of them.  Every row of M = d_mat = [N = 2^log_rows][width] is one leaf.
 * With t the permutation's width and D = t / 2 (the sponge's rate and the digest length, in base-field elements):
 * t = 16 on plans of 4-byte elements (NTT_FIELD_BABYBEAR, NTT_FIELD_KOALABEAR, NTT_PLAN_ELEM32), t = 8 on
 * NTT_FIELD_GOLDILOCKS: the shapes PaddingFreeSponge<Perm, t, D, D> and TruncatedPermutation<Perm, 2, D, t>.
 * The parameters are the caller's; the library ships no round constants and claims bit-compatibility with no
 * particular prover: that is a matter of the constants supplied.
 *   The permutation: M_E; rounds_f / 2 external rounds; rounds_p internal rounds; rounds_f / 2 external rounds.
 *     External round r: s_i += ext_rc[r][i]; s_i = s_i^a; s = M_E s.  M_E: M4 = [[2,3,1,1],[1,2,3,1],[1,1,2,3],
 *     [3,1,1,2]] on each group of four adjacent elements, then to every element the sum of the elements at the same
 *     position mod 4 over all groups (circ(2 M4, M4, .., M4)).  Internal round r: s_0 += int_rc[r]; s_0 = s_0^a;
 *     sigma = sum_i s_i; s_i = int_diag[i] s_i + sigma.
 *   The leaf hash of a row x_0..x_{width-1}: s = 0^t; for each chunk of up to D consecutive elements, overwrite
 *     s_0..s_{len-1} with it (the other positions stay as they are, for a short last chunk too) and permute; the
 *     digest is s_0..s_{D-1}.  Compression: s = left || right, permute, the digest is s_0..s_{D-1}.
 *   The tree: layer 0 is the N leaf digests in the order the rows are stored (a bit-reversed matrix gives a
 *     bit-reversed tree); node i of layer l is the compression of nodes 2i and 2i + 1 of layer l - 1.  d_tree is
 *     [2N - 1][D] elements, layer l starting at node 2N - 2^(L-l+1), L = log_rows; the root is node 2N - 2.  A cap
 *     is a layer of d_tree.
 * The matrix, the states and the digests are in the plan's I/O form: on NTT_PLAN_MONTGOMERY_IO plans they are the
 * Montgomery form of the same field elements (digest_mont = digest_canon 2^32 mod p).  The parameters are always
 * canonical host words.
 *   ntt_plan_set_poseidon2  width = t; sbox_degree a in {3, 5, 7} with gcd(a, p - 1) = 1; rounds_f even, 2..16;
 *     rounds_p 0..64 (int_rc may be NULL at 0); ext_rc [rounds_f][t], int_rc [rounds_p], int_diag [t].  Blocking,
 *     like plan creation; it must not race calls in flight on the plan; it may be called again to replace the
 *     parameters.  The plan keeps them in a device buffer of its own, allocated at the first call, its size
 *     independent of N.
 *   ntt_poseidon2_permute  d_states [count][t], permuted in place: the primitive, for transcripts and the caller's
 *     own sponges.  One launch.
 *   ntt_merkle_commit  d_tree from d_mat, which it leaves unmodified: one leaf launch (a lane a row, the rows of a
 *     workgroup through LDS, every element read once), one launch per layer (a lane a parent) down to 2^tail_log
 *     nodes, then one workgroup for the last tail_log layers through LDS.
 *   ntt_merkle_open  for query q with i = d_index[q] & (N - 1) (the indices live on the device; an index >= N
 *     wraps and nothing faults): d_rows[q] = row i of d_mat, and d_paths[q][l] = node (i >> l) ^ 1 of layer l, the
 *     sibling, l < log_rows.  d_mat and d_rows may both be NULL to skip the rows; d_paths may be NULL at
 *     log_rows 0, where a path is empty.  One launch.
 *   ntt_merkle_info  D, the elements of d_tree, the launches of ntt_merkle_commit and tail_log at (width,
 *     log_rows).  No launch; it needs no parameters.
 * A FRI layer: a fold output [M][d] in bit-reversed order, taken as [M >> k][d << k], has each fibre of the next
 * fold of arity 2^k as one row, so its commitment is ntt_merkle_commit with width = d << k and log_rows less k.
 * The three launching calls are asynchronous on hip_stream and never synchronise the host.  Any element-aligned
 * pointer is accepted; 16-byte accesses are used where the pointers (and the rows) are 16-byte aligned.
 * Engines: as the matrix calls; plans of fields 0-2 and of custom 4- and 6-limb moduli return NTT_ERR_ARG.
 * NTT_ERR_ARG before any launch, the buffers untouched: a null plan or pointer (but for the cases above), width 0,
 * N width >= 2^32, log_rows above the plan's log_n, nq 0, count 0, exactly one of d_mat and d_rows NULL, overlapping
 * byte ranges of an output with an input, NTT_PLAN_TWIDDLE_ONLY plans, a launching call before the parameters are
 * set; from ntt_plan_set_poseidon2: a width other than the engine's t, a degree outside {3, 5, 7} or sharing a
 * factor with p - 1, rounds_f odd or outside 2..16, rounds_p above 64, a parameter word >= p. */
int ntt_plan_set_poseidon2(ntt_plan* plan, unsigned width, unsigned sbox_degree, unsigned rounds_f, unsigned rounds_p,
                           const uint64_t* ext_rc, const uint64_t* int_rc, const uint64_t* int_diag);
int ntt_poseidon2_permute(ntt_plan* plan, void* d_states, uint64_t count, void* hip_stream);
int ntt_merkle_commit(ntt_plan* plan, const void* d_mat, unsigned width, unsigned log_rows, void* d_tree,
                      void* hip_stream);
int ntt_merkle_open(ntt_plan* plan, const void* d_mat, unsigned width, unsigned log_rows, const void* d_tree,
                    const uint32_t* d_index, unsigned nq, void* d_rows, void* d_paths, void* hip_stream);
int ntt_merkle_info(const ntt_plan* plan, unsigned width, unsigned log_rows, unsigned* digest_elems,
                    uint64_t* tree_elems, unsigned* launches, unsigned* tail_log);

/* Batch inversion and running sums / products down the columns of a row-major matrix: the second trace stage
 * between the first commitment and the second extension, the LogUp running-sum columns z_{i+1} = z_i + term_i and
 * the permutation argument's running products z_{i+1} = z_i ratio_i.  An extension element is d = ext_degree in
 * {1, 2, 4} adjacent base coefficients of F_p[X]/(X^d - W), W = ext_w, as in ntt_fri_fold.  Every buffer is in the
 * plan's I/O form (Montgomery on NTT_PLAN_MONTGOMERY_IO plans); ext_w is a canonical host word.
 *   ntt_batch_inverse  d_in, d_out [count][d]: d_out[i] = d_in[i]^-1 in the same form (v R goes to v^-1 R on
 *     Montgomery plans).  A zero element gives exactly zero and does not disturb its neighbours.  Montgomery's
 *     trick on runs: a thread multiplies up a run of 32 / d consecutive elements of 4 bytes (16 / d of 8 bytes),
 *     a zero counting as one, inverts the product once and walks back; the data reach the threads and leave them
 *     through LDS, 16 bytes a lane.  Where X^d - W is reducible and an element is a nonzero zero divisor, the
 *     outputs of that element's run are unspecified; nothing faults.  One launch.  d_out == d_in is allowed.
 *   ntt_matrix_scan  M = d_in = [rows][width] extension elements, row-major without pitch, any rows >= 1 (no table
 *     of the plan is used: rows may exceed the plan's n).  With (+) the field addition (op == NTT_SCAN_SUM) or the
 *     ring product (NTT_SCAN_PRODUCT): d_out[i][j] = (+)_{r <= i} M[r][j]; with flags & NTT_SCAN_EXCLUSIVE
 *     d_out[i][j] = (+)_{r < i} M[r][j] and d_out[0][j] is the identity: 0 for the sum; for the product 1 in the
 *     plan's I/O form in coordinate 0.  d_totals [width][d] (may be NULL) receives (+)_{all r} M[r][j] in both
 *     modes.  For the sum ext_w is ignored and the call is the scan of width d base columns.  Three launches:
 *     strips of adjacent columns x chunks of rows reduce into a plan-owned buffer [chunk][column][d] (allocated
 *     at the first use, its size independent of rows); the exclusive scan of the chunk aggregates per column and
 *     the totals; the chunks again, each scanned from its prefix.  One launch when there is one chunk.  Rows of
 *     at least 64 bytes: a strip is a power of two of columns, 64 to 256 bytes of a row.  Shorter rows: a chunk
 *     is one contiguous byte range that goes through LDS, 16 bytes a lane.  No atomics and no wait of one
 *     workgroup on another: the same bits every run.  d_out == d_in is allowed.
 *   ntt_scan_info  the decisions at (rows, width, ext_degree, op): the columns of a strip (for the sum: of the
 *     width d base columns), the consecutive rows a thread holds, the rows of a chunk, the chunks and the
 *     launches.  No launch.
 * The two launching calls are asynchronous on hip_stream and never synchronise the host.  Any element-aligned
 * pointer is accepted; 16-byte accesses are used when the pointers are 16-byte aligned and the buffers whole
 * 16-byte words long.
 * Engines: as the matrix calls; plans of fields 0-2 and of custom 4- and 6-limb moduli return NTT_ERR_ARG.
 * NTT_ERR_ARG before any launch, the buffers untouched: a null plan or pointer (d_totals may be NULL), count, rows
 * or width 0, count d or rows width d >= 2^32, ext_degree outside {1, 2, 4}, ext_w 0 or >= p when it is read
 * (ext_degree > 1, and not for the sum), an unknown op or flag bit, NTT_PLAN_TWIDDLE_ONLY plans, d_out overlapping
 * d_in other than d_out == d_in, d_totals overlapping d_in or d_out. */
#define NTT_SCAN_SUM 0u
#define NTT_SCAN_PRODUCT 1u
#define NTT_SCAN_EXCLUSIVE 1u
int ntt_batch_inverse(ntt_plan* plan, const void* d_in, void* d_out, uint64_t count, unsigned ext_degree,
                      uint64_t ext_w, void* hip_stream);
int ntt_matrix_scan(ntt_plan* plan, const void* d_in, void* d_out, uint64_t rows, unsigned width,
                    unsigned ext_degree, uint64_t ext_w, unsigned op, unsigned flags, void* d_totals,
                    void* hip_stream);
int ntt_scan_info(const ntt_plan* plan, uint64_t rows, unsigned width, unsigned ext_degree, unsigned op,
                  unsigned* strip_cols, unsigned* run_rows, unsigned* chunk_rows, unsigned* chunks,
                  unsigned* launches);

/* Pointwise product c = a * b mod p over 2^log_n elements (polynomial-multiply middle step);
 * a b R^-1 with NTT_PLAN_MONTGOMERY_IO. */
int ntt_pointwise_mul(ntt_plan* plan, const void* d_a, const void* d_b, void* d_c, void* hip_stream);
/* Cyclic polynomial product c = a * b of length 2^log_n: forward(a), forward(b), then the inverse
 * of their pointwise product into c (multi-pass 256-bit plans fuse the pointwise product into the
 * inverse's first pass).  a and b are overwritten with their transforms; c may alias a or b. */
int ntt_polymul(ntt_plan* plan, void* d_a, void* d_b, void* d_c, void* hip_stream);
/* Second half of a polymul over `batch` transforms laid out back to back: c = INTT(a * b) for a, b
 * already forward-transformed (fused into the inverse's first pass where the plan allows it).
 * c may alias a or b; a may equal b (squaring).  The distributed polymul runs it on each rank's
 * column-layout shares (ntt_polymul_multi, ntt_amd/distributed.py). */
int ntt_inverse_pointwise_batch(ntt_plan* plan, const void* d_a, const void* d_b, void* d_c, unsigned batch,
                                void* hip_stream);

/* Canonical-range check of a caller buffer (the contract every transform assumes: elements < p,
 * upper limbs zero).  The reference's only guard is CGBN's padded-store `BAD LIMB` trap
 * (impl_cuda.cu:1402-1408); this is a query instead: *bad = number of the `count` elements that are
 * not < p.  Blocking on hip_stream. */
int ntt_count_noncanonical(ntt_plan* plan, const void* d_data, uint64_t count, uint64_t* bad, void* hip_stream);

/* Fill a device vector with the SURVEY §8d synthetic inputs: kind 0 = x_j = j (the reference's
 * input, GZKP-NTT.cu:1587), kind 1 = SplitMix64 limbs with the top limb masked (seeded). */
int ntt_fill(ntt_plan* plan, void* d_data, int kind, uint64_t seed, void* hip_stream);

/* Fill `count` local elements: element i gets the synthetic value of global index
 * j = row0 + (i >> log_inner) + ((i mod 2^log_inner) << log_stride)  (log_inner >= 64: j = i).
 * Used to lay out one rank's share of a distributed vector. */
int ntt_fill_map(ntt_plan* plan, void* d_data, uint64_t count, int kind, uint64_t seed, uint64_t row0,
                 unsigned log_inner, unsigned log_stride, void* hip_stream);

/* ---------------------------------------------------------------- multi-GPU four-step, local steps
 * (the exchange itself is an RCCL all-to-all issued by the caller)
 * twiddle_pack: src = [2^log_rows][2^log_row_len] row-major; element (a, b) is multiplied by
 * w_n^((row0 + a) * b) (w_n^-1 if inverse; n = 2^log_n of the plan) and written to
 * dst[b >> log_block][a][b mod 2^log_block]: one contiguous chunk per destination rank.
 * transpose: dst[c][r] = src[r][c] for a 2^log_rows x 2^log_cols matrix of elements. */
int ntt_twiddle_pack(ntt_plan* plan, const void* d_src, void* d_dst, unsigned log_rows, unsigned log_row_len,
                     unsigned log_block, uint64_t row0, int inverse, void* hip_stream);
int ntt_transpose(ntt_plan* plan, const void* d_src, void* d_dst, unsigned log_rows, unsigned log_cols,
                  void* hip_stream);
/* The same with explicit chunk strides (several vectors exchanged in one all-to-all, e.g. the
 * distributed polymul's a and b): twiddle_pack writes peer chunk q at dst + q * peer_stride
 * elements (peer_stride >= 2^(log_rows + log_block)); transpose reads source rows in blocks of
 * 2^log_block_rows rows, block q starting at src + q * block_stride elements. */
int ntt_twiddle_pack_ex(ntt_plan* plan, const void* d_src, void* d_dst, unsigned log_rows, unsigned log_row_len,
                        unsigned log_block, uint64_t row0, int inverse, uint64_t peer_stride, void* hip_stream);
int ntt_transpose_ex(ntt_plan* plan, const void* d_src, void* d_dst, unsigned log_rows, unsigned log_cols,
                     unsigned log_block_rows, uint64_t block_stride, void* hip_stream);

/* Per-launch timing for benchmarks: when enabled, every transform records HIP events on its
 * stream between its kernel launches (a ring of 64 transforms, no host synchronisation);
 * ntt_plan_last_launch_ms returns per-launch durations (ms) averaged over the transforms recorded
 * since profiling was enabled (the last 64 at most), waiting for the most recent one; for the
 * schedule the most recent call ran (single-vector or batched, see ntt_plan_info). */
int ntt_plan_set_profiling(ntt_plan* plan, int enable);
int ntt_plan_last_launch_ms(ntt_plan* plan, float* ms, unsigned max_launches, unsigned* nlaunches);
/* The same launches' labels, comma-separated, in launch order: a kind letter and the pass's log2
 * radix (c column pass, "s" appended when it reads a Shoup-pair outer table; f final pass; s one
 * transform per workgroup; r several per workgroup; i in-place final pass with the digit reversal;
 * d digit-reversal swap; b single launch; n naive; x FRI fold, with log_arity for the radix; z DEEP points;
 * o open: strip sums, e open: the chunks and the scalars; a quotient: the alpha table, q quotient: the rows), ""
 * when unlabelled.  The Merkle calls: h leaf hash; m tree layers, with the number of layers the launch covers for
 * the radix; g open (gather); p permute.  The inverse and the scans: v batch inverse; t chunk totals, k the scan
 * of the totals, y the chunk scan.  NTT_ERR_ARG when `cap`
 * bytes do not hold them.  New (round 6): benchmarks pair per-launch PMC bytes with launches by
 * label, not by position. */
int ntt_plan_last_launch_labels(ntt_plan* plan, char* buf, unsigned cap);
/* Group mode: from this call on, the plan's transforms accumulate into ONE record (timings and
 * labels) until the next call, so that ntt_plan_last_launch_ms reports every launch of a caller-level
 * operation made of several transforms (the rank plan's row transforms of 2^15 rows each); the time
 * between two transforms of a group is not reported. */
int ntt_plan_profile_group(ntt_plan* plan);

/* Plan introspection: n, bytes per element, number of passes and their log2 radices (of a
 * single-vector transform: a default or Montgomery-I/O 4 x 64-bit plan of exactly 2^20 runs those on
 * 4096-element tiles in two passes, 10 + 10, and batched calls on 1024-element tiles, 7 + 7 + 6;
 * environment NTT_WIDE_TILES=0 keeps every call on the latter). */
int ntt_plan_info(const ntt_plan* plan, uint64_t* n, unsigned* elem_bytes, unsigned* npasses, unsigned radix_log[8]);
int ntt_plan_destroy(ntt_plan* plan);
const char* ntt_strerror(int status);

/* ---------------------------------------------------------------- reference-shaped shims */
/* SSIP(x, omega, log_n): P469762049 path, long long elements in device memory, blocking,
 * default stream (GZKP-NTT.cu:1452).  Prints nothing; errors are reported by the return value of
 * ntt_last_error(). */
void SSIP(long long* x, long long omega, unsigned log_n);
/* NTT_GZKP<8,256>(data, len, reverse, reverse_len, prime, omega, B, G) (big-num.cu:260): 256-bit
 * elements (8 x u32 LE), any odd prime < 2^255 given as 8 u32 words, omega = generator.  reverse /
 * reverse_len / B / G are accepted for signature compatibility and ignored (the transform is
 * self-sorting).  Blocking, default stream.  Returns a status. */
int NTT_GZKP_256(uint32_t* data, uint32_t len, const void* reverse, uint32_t reverse_len, const uint32_t prime[8],
                 const uint32_t omega[8], uint32_t B, uint32_t G);
/* NTT_GZKP(data, reverse, len, omega, B, G, reverse_num) for P469762049 (parallel-load.cu:195). */
int NTT_GZKP_64(long long* data, const void* reverse, long long len, long long omega, int B, int G,
                long long reverse_num);
int ntt_last_error(void);
/* The shims cache one plan per (modulus, generator, limbs, size, device) -- the reference rebuilt
 * its tables on every call (GZKP-NTT.cu:1476-1500, big-num.cu:278-309) -- keeping at most
 * NTT_SHIM_CACHE_PLANS (environment, default 8) and dropping the least recently used one beyond
 * that.  This releases every cached plan (a shim call still running keeps its plan until it returns). */
void ntt_shim_cache_clear(void);

/* ---------------------------------------------------------------- one rank of the distributed four-step
 * New (the reference has no multi-GPU code).  The local steps of rank `rank` of `world`
 * around the all-to-all, fused so that no separate twiddle, pack or transpose pass runs: the row
 * transforms' last pass applies w_n^(j1 k2) and stores straight into the peer chunks, and the column
 * transforms read the received chunks in place (2^log_c interleaved transforms).  Layouts as the
 * multi-GPU plan below: row layout [r][n2], column layout [n1][c]; the split n1 x n2 is the plan's
 * (ntt_rplan_info), the same for every rank of one (field, log_n, limbs64, world).  Send / receive buffers are the
 * caller's: [world][nvec][chunk] elements (chunk = r c, ntt_rplan_info), exchanged by the caller
 * as ONE all-to-all of equal chunks (RCCL, device copies, ...).  nvec = 2 carries two vectors per
 * exchange (polymul: slot 0 = a, slot 1 = b).  All calls are asynchronous on hip_stream. */
typedef struct ntt_rplan ntt_rplan;
int ntt_rplan_create(ntt_rplan** out, int field_id, unsigned log_n, unsigned limbs64, int world, int rank,
                     int device);
int ntt_rplan_info(const ntt_rplan* rp, uint64_t* local_n, uint64_t* chunk, unsigned* log_n1, unsigned* log_n2,
                   unsigned* elem_bytes);
/* row layout x (unchanged) -> send slot `slot` of nvec */
int ntt_rplan_forward_rows(ntt_rplan* rp, const void* d_x, void* d_send, unsigned nvec, unsigned slot,
                           void* hip_stream);
/* recv slot `slot` of nvec -> column layout x */
int ntt_rplan_forward_cols(ntt_rplan* rp, const void* d_recv, void* d_x, unsigned nvec, unsigned slot,
                           void* hip_stream);
/* column layout x (times y, pointwise, when y != NULL: the polymul's product) -> send (nvec = 1) */
int ntt_rplan_inverse_cols(ntt_rplan* rp, const void* d_x, const void* d_y, void* d_send, void* hip_stream);
/* recv (nvec = 1) -> row layout out (1/n included over both halves) */
int ntt_rplan_inverse_rows(ntt_rplan* rp, const void* d_recv, void* d_out, void* hip_stream);
/* The same two row steps over local rows [row0, row0 + nrows) only (1 <= nrows, row0 + nrows <= r).
 * Rows [row0, row0 + nrows) of every peer chunk form the contiguous run
 * [row0 c, (row0 + nrows) c) of that chunk, so a caller can exchange each piece as soon as it is written
 * (forward) or transform each piece as soon as it has arrived (inverse): the exchange of one piece
 * overlaps the row transforms of the next. */
int ntt_rplan_forward_rows_range(ntt_rplan* rp, const void* d_x, void* d_send, unsigned nvec, unsigned slot,
                                 uint64_t row0, uint64_t nrows, void* hip_stream);
int ntt_rplan_inverse_rows_range(ntt_rplan* rp, const void* d_recv, void* d_out, uint64_t row0, uint64_t nrows,
                                 void* hip_stream);
/* Pieces on BOTH sides of the exchange (ntt_amd/distributed.py FourStep): row_pieces P_r and
 * col_pieces P_c, powers of two (<= r and <= c); ra = r / P_r, cm = c / P_c.  Exchange blocks (one
 * per peer, nvec r c elements each) in these entry points' own layouts:
 *   forward [i][v][k][ra][cm]: forward_rows_piece(i) writes row piece i of vector `slot`;
 *     forward_cols_piece(k) transforms column piece k (columns k cm + [0, cm) of the column layout)
 *     once units (i, v, k) of every peer i have arrived -- row piece i of all vectors is one run
 *     [i nvec ra c, (i + 1) nvec ra c) of each block, unit (i, v, k) the run of ra cm elements at
 *     (i nvec + v) ra c + k ra cm;
 *   inverse [k][i][ra][cm]: inverse_cols_piece(k) (times y, same layout as x, if y != NULL) writes
 *     column piece k = the run [k r cm, (k + 1) r cm) of each block; inverse_rows_piece(i) transforms
 *     row piece i once the units (k, i) = runs of ra cm elements at k r cm + i ra cm have arrived.
 * So the exchange can overlap the row transforms before it and the column transforms after it
 * (forward), or the column transforms before it and the row transforms after it (inverse).  With
 * P_r = P_c = 1 the layouts are the [G][nvec][r][c] blocks above. */
int ntt_rplan_forward_rows_piece(ntt_rplan* rp, const void* d_x, void* d_send, unsigned nvec, unsigned slot,
                                 unsigned piece, unsigned row_pieces, unsigned col_pieces, void* hip_stream);
int ntt_rplan_forward_cols_piece(ntt_rplan* rp, const void* d_recv, void* d_x, unsigned nvec, unsigned slot,
                                 unsigned piece, unsigned row_pieces, unsigned col_pieces, void* hip_stream);
int ntt_rplan_inverse_cols_piece(ntt_rplan* rp, const void* d_x, const void* d_y, void* d_send, unsigned piece,
                                 unsigned row_pieces, unsigned col_pieces, void* hip_stream);
int ntt_rplan_inverse_rows_piece(ntt_rplan* rp, const void* d_recv, void* d_out, unsigned piece, unsigned row_pieces,
                                 unsigned col_pieces, void* hip_stream);
/* this rank's row-layout share of the global synthetic vector (kinds as ntt_fill) */
int ntt_rplan_fill(ntt_rplan* rp, void* d_x, int kind, uint64_t seed, void* hip_stream);
/* per-launch timing of the row (which = 0) or column (1) transforms, as ntt_plan_last_launch_ms */
int ntt_rplan_set_profiling(ntt_rplan* rp, int enable);
int ntt_rplan_last_launch_ms(ntt_rplan* rp, int which, float* ms, unsigned max_launches, unsigned* nlaunches);
int ntt_rplan_last_launch_labels(ntt_rplan* rp, int which, char* buf, unsigned cap);
/* the row and column plans' group mode (ntt_plan_profile_group): call at the start of every four-step
 * transform, so that the timings report each of its launches (e.g. the row transform's launches of
 * 2^15 rows each at world size 1) */
int ntt_rplan_profile_group(ntt_rplan* rp);
int ntt_rplan_destroy(ntt_rplan* rp);

/* ---------------------------------------------------------------- single-process multi-GPU
 * New (the reference has no multi-GPU code).  One plan drives `ngpus` devices of one node (power of
 * two); a transform is the four-step with ONE RCCL all-to-all over xGMI (ncclCommInitAll over
 * `devices`).  d_data[g] / hip_streams[g] belong to devices[g] (streams may be NULL = default
 * streams); each d_data[g] holds n / ngpus elements.  Device g runs ntt_rplan rank g.  Layouts (as
 * ntt_amd/distributed.py), with n = n1 n2, r = n1/ngpus, c = n2/ngpus, where the plan picks the split
 * (ntt_mplan_info / ntt_rplan_info): the fewest pass kernels, then the smallest largest radix, then
 * the most balanced split (2^24 on the 256-bit engines: n1 = 2^16, n2 = 2^8):
 *   forward input  (row layout):    d_data[g] = [r][n2], element (a, j2) = x[g r + a + n1 j2]
 *   forward output (column layout): d_data[g] = [n1][c], element (k1, kc) = X[g c + kc + n2 k1]
 * The inverse takes the column layout back to the row layout (1/n included).  Asynchronous.
 * NTT_FIELD_BABYBEAR and NTT_FIELD_KOALABEAR (4-byte elements) return NTT_ERR_ARG: the exchange
 * sizes count 8-byte words. */
typedef struct ntt_mplan ntt_mplan;
int ntt_mplan_create(ntt_mplan** out, int field_id, unsigned log_n, unsigned limbs64, int ngpus, const int* devices);
int ntt_forward_multi(ntt_mplan* plan, void* const* d_data, void* const* hip_streams);
int ntt_inverse_multi(ntt_mplan* plan, void* const* d_data, void* const* hip_streams);
/* Distributed cyclic polynomial product (BASELINE config 5): d_a[g], d_b[g] hold the
 * row-layout shares of a and b; on return d_c[g] holds the row-layout share of c = a * b (length n)
 * and d_a / d_b hold the column-layout shares of their forward transforms.  Forward(a) and
 * forward(b) share ONE all-to-all (each peer chunk carries both), the pointwise product is local
 * and fused into the inverse's first column pass, and the inverse's all-to-all brings c back to
 * the row layout: two exchanges for the three transforms.  d_c may alias d_a or d_b. */
int ntt_polymul_multi(ntt_mplan* plan, void* const* d_a, void* const* d_b, void* const* d_c, void* const* hip_streams);
/* each device's row-layout share of the global synthetic vector (kinds as ntt_fill) */
int ntt_mplan_fill(ntt_mplan* plan, void* const* d_data, int kind, uint64_t seed, void* const* hip_streams);
int ntt_mplan_info(const ntt_mplan* plan, uint64_t* local_n, unsigned* log_n1, unsigned* log_n2);
/* Pieces of the pipelined exchange on both sides (powers of two, <= 16, row_pieces <= r, col_pieces
 * <= c; the ntt_rplan_*_piece layouts): row piece i's exchange (grouped ncclSend / ncclRecv on a
 * per-device communication stream) overlaps the row transforms of piece i + 1, the last row piece
 * goes out per column piece and each column piece's transforms start when it has arrived (the
 * inverse mirrors it).  Default: 1 x 1, one whole-block exchange per transform (the pieces have
 * not yet measured a gain). */
int ntt_mplan_set_pieces2(ntt_mplan* plan, unsigned row_pieces, unsigned col_pieces);
/* Row pieces only (1..16, <= r; rounded down to a power of two), one column piece. */
int ntt_mplan_set_pieces(ntt_mplan* plan, unsigned pieces);
int ntt_mplan_destroy(ntt_mplan* plan);

#ifdef __cplusplus
}
#endif
#endif
