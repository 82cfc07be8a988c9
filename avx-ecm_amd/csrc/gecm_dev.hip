// gecm_dev.hip — device management for libgecm (gfx950 / MI355X only): buffers, stream, events,
// dispatch to the kernel launchers of gecm_kernels.hip through the two tables of the limb count (gecm_launch.h).
#include "gecm_dev.h"
#include "gecm_launch.h"
#include "gecm_tape.h"
#include <hip/hip_runtime.h>
#include <array>
#include <cstdlib>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

static thread_local std::string g_err;
extern "C" const char *gecm_dev_error(void) { return g_err.c_str(); }

#define HIPCHK(x)                                                                             \
    do {                                                                                      \
        hipError_t e_ = (x);                                                                  \
        if (e_ != hipSuccess) {                                                               \
            char b_[512];                                                                     \
            snprintf(b_, sizeof b_, "%s failed: %s (%s:%d)", #x, hipGetErrorString(e_), __FILE__, __LINE__); \
            g_err = b_;                                                                       \
            return -1;                                                                        \
        }                                                                                     \
    } while (0)

// ---------------------------------------------------------------- host side
// the kernel tables of every built limb count (gecm_kernels.hip: one accessor per object)
struct nl_kernels {
    int nl;
    const gecm_kernels_p1 *(*p1)(void);
    const gecm_kernels_p2 *(*p2)(void);
};
static const nl_kernels k_kernels[] = {
#define X(n) {n, gecm_kernels_##n##_p1, gecm_kernels_##n##_p2},
    GECM_NL_LIST(X)
#undef X
};

static const nl_kernels *kernels_for(int nl)
{
    for (const auto &k : k_kernels)
        if (k.nl == nl) return &k;
    return nullptr;
}

extern "C" const int *gecm_dev_supported_nl(void)
{
    static const auto nls = [] {
        std::array<int, sizeof k_kernels / sizeof k_kernels[0] + 1> a{};   // zero-terminated
        for (size_t i = 0; i + 1 < a.size(); i++) a[i] = k_kernels[i].nl;
        return a;
    }();
    return nls.data();
}

#ifndef GECM_S2_WAVES_PER_SIMD
#define GECM_S2_WAVES_PER_SIMD 16         // wavefronts per SIMD a pair-walk launch is cut up for (gecm_dev_s2_init)
#endif
#define GECM_S2_MAX_SLICES 64
// Constant sets of a row kernel in device memory, one per modulus: `sets` of them (0 = not available), for nq limbs per
// lane and `rows` rows of a multiply.
struct row_consts {
    uint32_t *d = nullptr;
    size_t cap = 0;
    uint32_t sets = 0;
    int nq = 0, rows = 0;
};
struct gecm_dev {
    int device = 0;
    int nl = 0;
    const gecm_kernels_p1 *k1 = nullptr;   // the launchers of this limb count
    const gecm_kernels_p2 *k2 = nullptr;
    gecm_devmod mod = {};            // the context's modulus (gecm_dev_open), its pointers into mod_limbs
    std::vector<uint32_t> mod_limbs;
    size_t ncurves = 0, stride = 0;
    uint32_t *dX = nullptr, *dZ = nullptr, *dS = nullptr, *dT0 = nullptr, *dT1 = nullptr;
    uint32_t *dTape = nullptr;
    size_t tape_len = 0, tape_cap = 0;
    std::vector<hipEvent_t> cut_events;   // one per stage-1 launch of the last gecm_dev_stage1 (progress of a long tape)
    size_t cut_launches = 0;
    std::vector<size_t> tape_cuts;   // byte offsets at which a stage-1 launch may start (gecm_dev_set_tape), first = 0, last = tape_len
    // stage 2
    uint32_t *dPbX = nullptr, *dBlk = nullptr, *dPd = nullptr, *dAcc = nullptr, *dFail = nullptr, *dKeep = nullptr;
    uint32_t *dPa = nullptr, *dSteps = nullptr, *dFlags = nullptr;
    size_t flags_cap = 0;
    size_t s2_npb = 0, s2_G = 0, s2_ring = 0, s2_stride = 0, steps_cap = 0, keep_cap = 0;
    uint64_t steps_id = 0;    // the kept tape whose copy dSteps holds (0: none), and its length
    uint32_t steps_n = 0;
    uint32_t s2_slices = 1;   // stage-2 accumulators per curve (pair-walk slices), see gecm_dev_s2_init
    uint32_t s2_K = 1;        // sub-sequences per curve for the table build and the giant steps (gecm_dev_s2_subseq)
    int s2_subseq_set = 0;    // gecm_dev_set_s2_subseq: 0 = default, -1 = by batch size on every kind of context, or K itself
    uint32_t s2_k_chunks = 0; // giant-step chunks launched with sub-sequences since the last gecm_dev_s2_init
    uint32_t *dKBlk = nullptr, *dKPa = nullptr, *dPdK = nullptr, *dTgt = nullptr;
    size_t tgt_cap = 0;
    hipStream_t stream = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    float last_ms = 0.f;
    bool timed = false;
    uint32_t *dModQ = nullptr;   // N and K' limbs padded to 40 each, for the eight-lane kernel
    // constant sets of the row kernels (set_row_consts): the 32-lane kernel's one set of a single N (gecm_dev_set_rowconst),
    // the 16-lane method kernel's (_set_unit_rowconst) and the 32-lane kernel's on a multi-modulus batch (_set_multi_rowconst)
    row_consts rowc, urowc, mrowc;
    int fform = 0;       // +1 / -1 / 2: modulus is 2^k - 1 / 2^k + 1 / 2^k - c and stage 1 uses the special multiply (gecm_dev_set_fform)
    int cus = 0;          // compute units of the device (4 SIMDs each)
    int last_lanes = 0;   // lanes per curve the last stage-1 launch used
    std::string last_kernel;   // and the kernel's name as rocprofv3 prints it
    // multi-modulus context (gecm_dev_open): one modulus per 64-curve block, constants in device memory
    bool wide = false;    // gecm_dev_open_wide: no kernel tables (k1, k2 stay null), the 32-lane kernel of the wide shapes only
    bool multi = false;
    unsigned char *dGroups = nullptr; // one packed constant set per modulus (gecm_kernels_p1::pack_group)
    uint32_t *dBlockGroup = nullptr;  // modulus of every 64-curve block of the batch
    size_t groups_cap = 0, blocks_cap = 0;
    bool have_groups = false;
    uint32_t ngroups = 0;             // moduli of the batch (gecm_dev_set_groups)
    // lane packing (gecm_dev_set_groups with curve_group): one modulus per curve position instead of one per block
    uint32_t *dCurveGroup = nullptr;
    size_t curve_group_cap = 0;
    bool lane_packed = false;
    // curve construction on the device (gecm_dev_build)
    uint64_t *dSigma = nullptr;
    size_t sigma_cap = 0;
    uint8_t *dParam = nullptr;        // the parametrisation of every curve position (gecm_dev_build_param)
    size_t param_cap = 0;
    float build_ms = 0.f;
};

// ---- source manifest (Makefile): "K:<hash of the kernel objects' sources, or MIXED> R:<rowk> D:<this file>"
#ifndef GECM_MANIFEST
#define GECM_MANIFEST "unset"
#endif
extern "C" const char *gecm_manifest_rowk(void);
extern "C" const char *gecm_manifest_rowk_wide(void);
extern "C" const char *gecm_dev_manifest(void)
{
    static std::string m;
    if (m.empty()) {
        std::string k;
        bool mixed = false;
        for (const auto &kt : k_kernels)
            for (const char *h : {kt.p1()->manifest, kt.p2()->manifest}) {
                if (k.empty()) k = h;
                else if (k != h) mixed = true;
            }
        std::string t = std::string("K:") + (mixed ? "MIXED" : k) + " R:" +
                        (strcmp(gecm_manifest_rowk(), gecm_manifest_rowk_wide()) ? "MIXED" : gecm_manifest_rowk()) + " D:" + GECM_MANIFEST;
#ifdef GECM_DEV_NL15
        t += " DEV-BUILD(416-bit class only)";
#endif
        m = t;
    }
    return m.c_str();
}

extern "C" int gecm_dev_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

static gecm_modconst modconst(const gecm_dev *d)
{
    gecm_modconst mc;
    mc.m = d->mod;
    mc.source = !d->multi ? GECM_SRC_VALUE : d->lane_packed ? GECM_SRC_LANE : GECM_SRC_WAVE;
    mc.groups = d->multi ? d->dGroups : nullptr;
    mc.block_group = d->multi ? d->dBlockGroup : nullptr;
    mc.curve_group = mc.source == GECM_SRC_LANE ? d->dCurveGroup : nullptr;
    return mc;
}

// Has the context what operation `fn` needs?  NEEDS_TABLE: a kernel table of the limb count, which a wide context
// (gecm_dev_open_wide) has not.  NEEDS_BATCH: a batch, and on a multi-modulus context the batch's moduli.  NEEDS_R3: those,
// and r3 (the operation inverts).  Asked for together, they are looked at in that order.
enum : unsigned { NEEDS_TABLE = 1, NEEDS_BATCH = 2, NEEDS_R3 = 4 };
static int ready(const gecm_dev *d, const char *fn, unsigned needs)
{
    const char *lacks = (needs & NEEDS_TABLE) && d->wide       ? "not available on a wide context (gecm_dev_open_wide)"
                        : !(needs & (NEEDS_BATCH | NEEDS_R3))  ? nullptr
                        : !d->stride                           ? "no batch (gecm_dev_resize)"
                        : d->multi && !d->have_groups          ? "the moduli of the batch are not set (gecm_dev_set_groups)"
                        : (needs & NEEDS_R3) && !d->mod.r3     ? "the context was opened without inversion constants (r3)"
                                                               : nullptr;
    if (!lacks) return 0;
    g_err = std::string(fn) + ": " + lacks;
    return -2;
}

// A device array that only grows: room for `want` elements at *p, of which *cap says how many it has.  What it held is
// not kept.
template <class T>
static int grow(T **p, size_t *cap, size_t want)
{
    if (want <= *cap) return 0;
    (void)hipFree(*p);
    *p = nullptr;
    *cap = 0;
    HIPCHK(hipMalloc(p, want * sizeof(T)));
    *cap = want;
    return 0;
}

// What every context starts from: the device checked and made current, its compute units, the stream and the two events.
// fn names the caller in the error text.
static int open_common(gecm_dev **out, const char *fn, int device, int nl)
{
    int cnt = 0;
    HIPCHK(hipGetDeviceCount(&cnt));
    if (device < 0 || device >= cnt) {
        g_err = std::string(fn) + ": no such device";
        return -2;
    }
    HIPCHK(hipSetDevice(device));
    int cus = 0;
    HIPCHK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device));
    gecm_dev *d = new gecm_dev;
    d->device = device;
    d->cus = cus;
    d->nl = nl;
    HIPCHK(hipStreamCreateWithFlags(&d->stream, hipStreamNonBlocking));
    HIPCHK(hipEventCreate(&d->ev0));
    HIPCHK(hipEventCreate(&d->ev1));
    *out = d;
    return 0;
}

extern "C" int gecm_dev_open(gecm_dev **out, int device, int nl, const gecm_devmod *m, int multi)
{
    const auto *kt = kernels_for(nl);
    if (!kt) {
        g_err = "gecm_dev_open: unsupported limb count " + std::to_string(nl);
        return -2;
    }
    if (!m || !m->n || !m->kp || !m->one || !m->r2) {
        g_err = "gecm_dev_open: the modulus constants are incomplete";
        return -2;
    }
    gecm_dev *d = nullptr;
    if (const int rc = open_common(&d, "gecm_dev_open", device, nl)) return rc;
    d->k1 = kt->p1();
    d->k2 = kt->p2();
    d->multi = multi != 0;
    const uint32_t *rows[5] = {m->n, m->kp, m->one, m->r2, m->r3};
    d->mod_limbs.assign((size_t)5 * nl, 0);
    uint32_t *own[5];
    for (int q = 0; q < 5; q++) {
        own[q] = d->mod_limbs.data() + (size_t)q * nl;
        if (rows[q]) memcpy(own[q], rows[q], (size_t)nl * sizeof(uint32_t));
    }
    d->mod = {own[0], own[1], own[2], own[3], m->r3 ? own[4] : nullptr, m->rho, m->inv_iters};
    if (nl <= 40) {
        uint32_t h[80] = {0};
        for (int i = 0; i < nl; i++) {
            h[i] = m->n[i];
            h[40 + i] = m->kp[i];
        }
        HIPCHK(hipMalloc(&d->dModQ, sizeof h));
        HIPCHK(hipMemcpy(d->dModQ, h, sizeof h, hipMemcpyHostToDevice));
    }
    *out = d;
    return 0;
}

// A wide context (gecm_dev.h): a limb count of the wide shapes, which kernels_for() does not know.  It has rho; the row
// kernel's constants come with gecm_dev_set_rowconst.
extern "C" int gecm_dev_open_wide(gecm_dev **out, int device, int nl, uint32_t rho)
{
    bool shape = false;
#define X(q, r) shape |= nl + 1 == r;
    GECM_ROW_WIDE_SHAPES(X)
#undef X
    if (!shape || kernels_for(nl)) {
        g_err = "gecm_dev_open_wide: " + std::to_string(nl) + " limbs is not a limb count of the wide shapes";
        return -2;
    }
    if (const int rc = open_common(out, "gecm_dev_open_wide", device, nl)) return rc;
    (*out)->wide = true;
    (*out)->mod.rho = rho;
    return 0;
}

extern "C" int gecm_dev_is_wide(const gecm_dev *d) { return d && d->wide; }

// `sets` constant sets of set_words words each into a store, for nq limbs per lane and `rows` rows of a multiply.
// Synchronous: the host array may go away when this returns.
static int set_row_consts(gecm_dev *d, const char *fn, row_consts *store, size_t set_words, uint32_t sets, int nq, int rows,
                          const uint32_t *words)
{
    HIPCHK(hipSetDevice(d->device));
    if (nq < 1 || nq > GECM_ROW_MAXNQ || 16 * nq > GECM_ROW_WORDS || rows <= 16 * (nq - 1) || rows > 16 * nq || !sets || !words) {
        g_err = std::string(fn) + ": limbs per lane out of range, or no constants";
        return -2;
    }
    store->sets = 0;
    if (grow(&store->d, &store->cap, sets * set_words)) return -1;
    HIPCHK(hipMemcpyAsync(store->d, words, sets * set_words * sizeof(uint32_t), hipMemcpyHostToDevice, d->stream));
    HIPCHK(hipStreamSynchronize(d->stream));
    store->nq = nq;
    store->rows = rows;
    store->sets = sets;
    return 0;
}

extern "C" int gecm_dev_set_rowconst(gecm_dev *d, int nq, int rows, const uint32_t *words)
{
    if (d->wide && (nq != 3 || rows != d->nl + 1)) {
        g_err = "gecm_dev_set_rowconst: a wide context takes three limbs per lane and its own limb count + 1 rows";
        return -2;
    }
    return set_row_consts(d, "gecm_dev_set_rowconst", &d->rowc, GECM_ROW_KINDS * GECM_ROW_WORDS, 1, nq, rows, words);
}

extern "C" int gecm_dev_set_unit_rowconst(gecm_dev *d, int nq, int rows, uint32_t ngroups, const uint32_t *words)
{
    if (ready(d, "gecm_dev_set_unit_rowconst", NEEDS_TABLE)) return -2;
    return set_row_consts(d, "gecm_dev_set_unit_rowconst", &d->urowc, GECM_UROW_SET, ngroups, nq, rows, words);
}

extern "C" int gecm_dev_set_multi_rowconst(gecm_dev *d, int nq, int rows, uint32_t ngroups, const uint32_t *words)
{
    if (ready(d, "gecm_dev_set_multi_rowconst", NEEDS_TABLE)) return -2;
    if (!d->multi) {
        g_err = "gecm_dev_set_multi_rowconst: not a multi-modulus context";
        return -2;
    }
    return set_row_consts(d, "gecm_dev_set_multi_rowconst", &d->mrowc, GECM_MROW_SET, ngroups, nq, rows, words);
}

extern "C" int gecm_dev_cus(gecm_dev *d) { return d->cus; }

// are there sets in the store for the moduli of the batch?
static bool row_consts_ready(const gecm_dev *d, const row_consts &store)
{
    return store.sets != 0 && store.sets == (d->multi ? d->ngroups : 1u);
}

extern "C" int gecm_dev_multi_rows_ready(gecm_dev *d) { return d->multi && row_consts_ready(d, d->mrowc); }
extern "C" int gecm_dev_unit_rows_ready(gecm_dev *d) { return row_consts_ready(d, d->urowc); }

static void free_state(gecm_dev *d)
{
    (void)hipFree(d->dX); (void)hipFree(d->dZ); (void)hipFree(d->dS); (void)hipFree(d->dT0); (void)hipFree(d->dT1);
    d->dX = d->dZ = d->dS = d->dT0 = d->dT1 = nullptr;
}

static void free_s2(gecm_dev *d)
{
    (void)hipFree(d->dPbX); (void)hipFree(d->dBlk); (void)hipFree(d->dPd); (void)hipFree(d->dAcc);
    (void)hipFree(d->dFail); (void)hipFree(d->dPa);
    (void)hipFree(d->dKBlk); (void)hipFree(d->dKPa); (void)hipFree(d->dPdK);
    d->dKBlk = d->dKPa = d->dPdK = nullptr;
    d->dPbX = d->dBlk = d->dPd = d->dAcc = d->dFail = d->dPa = nullptr;
    d->s2_npb = d->s2_G = d->s2_ring = d->s2_stride = 0;
}

extern "C" void gecm_dev_close(gecm_dev *d)
{
    if (!d) return;
    for (hipEvent_t e : d->cut_events) (void)hipEventDestroy(e);
    (void)hipSetDevice(d->device);
    free_state(d);
    free_s2(d);
    (void)hipFree(d->dModQ);
    for (row_consts *store : {&d->rowc, &d->urowc, &d->mrowc}) (void)hipFree(store->d);
    (void)hipFree(d->dKeep);
    (void)hipFree(d->dSteps);
    (void)hipFree(d->dFlags);
    (void)hipFree(d->dTape);
    (void)hipFree(d->dGroups);
    (void)hipFree(d->dBlockGroup);
    (void)hipFree(d->dCurveGroup);
    (void)hipFree(d->dSigma);
    (void)hipFree(d->dParam);
    if (d->ev0) (void)hipEventDestroy(d->ev0);
    if (d->ev1) (void)hipEventDestroy(d->ev1);
    if (d->stream) (void)hipStreamDestroy(d->stream);
    delete d;
}

extern "C" int gecm_dev_memory(gecm_dev *d, uint64_t *free_bytes, uint64_t *total_bytes)
{
    HIPCHK(hipSetDevice(d->device));
    size_t f = 0, t = 0;
    HIPCHK(hipMemGetInfo(&f, &t));
    if (free_bytes) *free_bytes = f;
    if (total_bytes) *total_bytes = t;
    return 0;
}

extern "C" int gecm_dev_device_name(gecm_dev *d, char *buf, size_t len)
{
    hipDeviceProp_t p;
    HIPCHK(hipGetDeviceProperties(&p, d->device));
    /* (some boxes report an empty marketing name) */
    snprintf(buf, len, "%s (%s, %d CUs)", p.name[0] ? p.name : "AMD GPU", p.gcnArchName, p.multiProcessorCount);
    return 0;
}

extern "C" size_t gecm_dev_stride(gecm_dev *d) { return d->stride; }

extern "C" int gecm_dev_resize(gecm_dev *d, size_t ncurves)
{
    HIPCHK(hipSetDevice(d->device));
    size_t stride = (ncurves + 63) / 64 * 64;
    if (stride == 0) stride = 64;
    if (stride != d->stride) {
        free_state(d);
        size_t bytes = stride * d->nl * sizeof(uint32_t);
        HIPCHK(hipMalloc(&d->dX, bytes));
        HIPCHK(hipMalloc(&d->dZ, bytes));
        HIPCHK(hipMalloc(&d->dS, bytes));
        if (!d->wide) {                        // the scratch planes of the downloads: a wide context has none
            HIPCHK(hipMalloc(&d->dT0, bytes));
            HIPCHK(hipMalloc(&d->dT1, bytes));
        }
        d->stride = stride;
    }
    d->ncurves = ncurves;
    d->have_groups = false;
    d->lane_packed = false;
    return 0;
}

// host [limb][ncurves] -> device [limb][stride], padding lanes zero
static int upload_soa(gecm_dev *d, uint32_t *dst, const uint32_t *src)
{
    HIPCHK(hipMemsetAsync(dst, 0, d->stride * d->nl * sizeof(uint32_t), d->stream));
    if (d->ncurves)
        HIPCHK(hipMemcpy2DAsync(dst, d->stride * 4, src, d->ncurves * 4, d->ncurves * 4, d->nl,
                                hipMemcpyHostToDevice, d->stream));
    return 0;
}

static int download_soa(gecm_dev *d, uint32_t *dst, const uint32_t *src)
{
    if (d->ncurves)
        HIPCHK(hipMemcpy2DAsync(dst, d->ncurves * 4, src, d->stride * 4, d->ncurves * 4, d->nl,
                                hipMemcpyDeviceToHost, d->stream));
    return 0;
}

extern "C" int gecm_dev_upload(gecm_dev *d, const uint32_t *X, const uint32_t *Z, const uint32_t *S)
{
    HIPCHK(hipSetDevice(d->device));
    if (upload_soa(d, d->dX, X)) return -1;
    if (upload_soa(d, d->dZ, Z)) return -1;
    if (upload_soa(d, d->dS, S)) return -1;
    HIPCHK(hipStreamSynchronize(d->stream));
    return 0;
}

extern "C" int gecm_dev_upload_xz(gecm_dev *d, const uint32_t *X, const uint32_t *Z)
{
    if (ready(d, "gecm_dev_upload_xz", NEEDS_TABLE)) return -2;
    HIPCHK(hipSetDevice(d->device));
    if (upload_soa(d, d->dX, X)) return -1;
    if (upload_soa(d, d->dZ, Z)) return -1;
    HIPCHK(hipStreamSynchronize(d->stream));
    return 0;
}

// Plain residues into the batch: x, z canonical in [0, N), host [limb][ncurves]; X = x R mod N, Z = z R mod N by the
// to_mont kernel, through the scratch planes the downloads use.  The padding lanes get x = z = 1.
extern "C" int gecm_dev_upload_plain(gecm_dev *d, const uint32_t *x, const uint32_t *z)
{
    if (ready(d, "gecm_dev_upload_plain", NEEDS_TABLE | NEEDS_BATCH)) return -2;
    HIPCHK(hipSetDevice(d->device));
    if (upload_soa(d, d->dT0, x)) return -1;
    if (upload_soa(d, d->dT1, z)) return -1;
    const size_t pad = d->stride - d->ncurves;        // at most 63: limb 0 of the padding lanes, set to 1
    const std::vector<uint32_t> ones(pad ? pad : 1, 1u);
    if (pad) {
        HIPCHK(hipMemcpyAsync(d->dT0 + d->ncurves, ones.data(), pad * sizeof(uint32_t), hipMemcpyHostToDevice, d->stream));
        HIPCHK(hipMemcpyAsync(d->dT1 + d->ncurves, ones.data(), pad * sizeof(uint32_t), hipMemcpyHostToDevice, d->stream));
    }
    gecm_modconst mc = modconst(d);
    d->k1->to_mont(d->stream, &mc, d->dT0, d->dT1, d->dX, d->dZ, d->stride);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(d->stream));
    return 0;
}

extern "C" int gecm_dev_download_s(gecm_dev *d, uint32_t *S)
{
    if (ready(d, "gecm_dev_download_s", NEEDS_TABLE)) return -2;
    HIPCHK(hipSetDevice(d->device));
    if (!d->stride) {
        g_err = "gecm_dev_download_s: no batch";
        return -2;
    }
    if (download_soa(d, S, d->dS)) return -1;
    HIPCHK(hipStreamSynchronize(d->stream));
    return 0;
}

// ---------------------------------------------------------------- curve construction
extern "C" float gecm_dev_last_build_ms(gecm_dev *d) { return d->build_ms; }

// The end of gecm_dev_build, _build_param and _normalize, whose kernels ev0 precedes: their time into build_ms and the
// flags of `count` positions to the host.  Synchronous.
static int timed_flags(gecm_dev *d, uint32_t *flags, size_t count)
{
    HIPCHK(hipEventRecord(d->ev1, d->stream));
    HIPCHK(hipMemcpyAsync(flags, d->dFlags, count * 4, hipMemcpyDeviceToHost, d->stream));
    HIPCHK(hipStreamSynchronize(d->stream));
    HIPCHK(hipEventElapsedTime(&d->build_ms, d->ev0, d->ev1));
    d->timed = false;
    return 0;
}

extern "C" int gecm_dev_build(gecm_dev *d, const uint64_t *sigma, size_t count, uint32_t *flags)
{
    if (ready(d, "gecm_dev_build", NEEDS_TABLE)) return -2;
    HIPCHK(hipSetDevice(d->device));
    if (!d->stride || count != d->ncurves || !sigma || !flags) {
        g_err = "gecm_dev_build: no batch of that many curves (gecm_dev_resize)";
        return -2;
    }
    if (ready(d, "gecm_dev_build", NEEDS_R3)) return -2;
    if (grow(&d->dSigma, &d->sigma_cap, d->stride) || grow(&d->dFlags, &d->flags_cap, d->stride)) return -1;
    // the padding lanes build sigma = 0: computed, never flagged or read
    HIPCHK(hipMemsetAsync(d->dSigma, 0, d->stride * sizeof(uint64_t), d->stream));
    HIPCHK(hipMemcpyAsync(d->dSigma, sigma, count * sizeof(uint64_t), hipMemcpyHostToDevice, d->stream));
    gecm_modconst mc = modconst(d);
    HIPCHK(hipEventRecord(d->ev0, d->stream));
    d->k1->build(d->stream, &mc, d->dSigma, d->dX, d->dZ, d->dS, d->dFlags, d->stride);
    HIPCHK(hipGetLastError());
    return timed_flags(d, flags, count);
}

extern "C" int gecm_dev_build_param(gecm_dev *d, const uint64_t *sigma, const uint8_t *param, size_t count, uint32_t *flags)
{
    if (ready(d, "gecm_dev_build_param", NEEDS_TABLE)) return -2;
    HIPCHK(hipSetDevice(d->device));
    if (!d->stride || count != d->ncurves || !sigma || !param || !flags) {
        g_err = "gecm_dev_build_param: no batch of that many curves (gecm_dev_resize)";
        return -2;
    }
    bool suyama = false, other = false;
    for (size_t i = 0; i < count; i++) {
        if (param[i] != 0 && param[i] != 1 && param[i] != 3) {
            g_err = "gecm_dev_build_param: a parametrisation other than 0, 1 and 3";
            return -2;
        }
        (param[i] ? other : suyama) = true;
    }
    if (ready(d, "gecm_dev_build_param", suyama ? NEEDS_R3 : NEEDS_BATCH)) return -2;
    if (grow(&d->dSigma, &d->sigma_cap, d->stride) || grow(&d->dFlags, &d->flags_cap, d->stride) ||
        grow(&d->dParam, &d->param_cap, d->stride))
        return -1;
    // the padding lanes: sigma = 0 with parameter 0, computed by k_build (if it runs), never flagged or read
    HIPCHK(hipMemsetAsync(d->dSigma, 0, d->stride * sizeof(uint64_t), d->stream));
    HIPCHK(hipMemcpyAsync(d->dSigma, sigma, count * sizeof(uint64_t), hipMemcpyHostToDevice, d->stream));
    HIPCHK(hipMemsetAsync(d->dParam, 0, d->stride, d->stream));
    HIPCHK(hipMemcpyAsync(d->dParam, param, count, hipMemcpyHostToDevice, d->stream));
    if (!suyama) {
        // no k_build: what it would have written in the lanes k_build_param leaves alone is cleared instead
        const size_t plane = (size_t)d->nl * d->stride * sizeof(uint32_t);
        HIPCHK(hipMemsetAsync(d->dX, 0, plane, d->stream));
        HIPCHK(hipMemsetAsync(d->dZ, 0, plane, d->stream));
        HIPCHK(hipMemsetAsync(d->dS, 0, plane, d->stream));
        HIPCHK(hipMemsetAsync(d->dFlags, 0, d->stride * sizeof(uint32_t), d->stream));
    }
    gecm_modconst mc = modconst(d);
    HIPCHK(hipEventRecord(d->ev0, d->stream));
    if (suyama) d->k1->build(d->stream, &mc, d->dSigma, d->dX, d->dZ, d->dS, d->dFlags, d->stride);
    HIPCHK(hipGetLastError());
    if (other) d->k1->build_param(d->stream, &mc, d->dSigma, d->dParam, d->dX, d->dZ, d->dS, d->dFlags, d->stride);
    HIPCHK(hipGetLastError());
    return timed_flags(d, flags, count);
}

extern "C" int gecm_dev_normalize(gecm_dev *d, uint32_t *flags)
{
    if (ready(d, "gecm_dev_normalize", NEEDS_TABLE | NEEDS_R3)) return -2;
    HIPCHK(hipSetDevice(d->device));
    if (!d->ncurves || !flags) {
        g_err = "gecm_dev_normalize: no curves, or nowhere to put their flags";
        return -2;
    }
    if (grow(&d->dFlags, &d->flags_cap, d->stride)) return -1;
    gecm_modconst mc = modconst(d);
    HIPCHK(hipEventRecord(d->ev0, d->stream));
    d->k1->normalize(d->stream, &mc, d->dX, d->dZ, d->dFlags, d->stride);
    HIPCHK(hipGetLastError());
    return timed_flags(d, flags, d->ncurves);
}

extern "C" int gecm_dev_fill_twin(gecm_dev *dst, gecm_dev *src)
{
    if (ready(dst, "gecm_dev_fill_twin", NEEDS_TABLE) || ready(src, "gecm_dev_fill_twin", NEEDS_TABLE)) return -2;
    HIPCHK(hipSetDevice(src->device));
    if (dst->device != src->device || !src->stride || dst->stride != src->stride || dst->ncurves != src->ncurves ||
        src->multi || dst->multi) {
        g_err = "gecm_dev_fill_twin: the two contexts do not hold batches of one size on one device";
        return -2;
    }
    HIPCHK(hipStreamSynchronize(dst->stream));    // the copies below run on src's stream
    const int common = src->nl < dst->nl ? src->nl : dst->nl;
    const size_t row = src->stride * sizeof(uint32_t);
    const gecm_modconst ms = modconst(src), md = modconst(dst);
    // src's planes out of Montgomery form into its scratch planes, then limb plane by limb plane into dst's
    auto lift = [&](const uint32_t *a, const uint32_t *b) -> int {
        src->k1->from_mont(src->stream, &ms, a, b, src->dT0, src->dT1, src->stride);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemsetAsync(dst->dT0, 0, row * dst->nl, src->stream));
        HIPCHK(hipMemsetAsync(dst->dT1, 0, row * dst->nl, src->stream));
        HIPCHK(hipMemcpyAsync(dst->dT0, src->dT0, row * common, hipMemcpyDeviceToDevice, src->stream));
        HIPCHK(hipMemcpyAsync(dst->dT1, src->dT1, row * common, hipMemcpyDeviceToDevice, src->stream));
        HIPCHK(hipStreamSynchronize(src->stream));
        return 0;
    };
    if (lift(src->dX, src->dZ)) return -1;
    dst->k1->to_mont(dst->stream, &md, dst->dT0, dst->dT1, dst->dX, dst->dZ, dst->stride);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(dst->stream));
    if (lift(src->dS, src->dS)) return -1;
    // S twice: the kernel makes two planes at a time, the second copy goes to the scratch plane it does not read
    dst->k1->to_mont(dst->stream, &md, dst->dT0, dst->dT0, dst->dS, dst->dT1, dst->stride);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(dst->stream));
    return 0;
}

extern "C" int gecm_dev_set_tape(gecm_dev *d, const uint8_t *tape, size_t len)
{
    HIPCHK(hipSetDevice(d->device));
    size_t words = (len + 3) / 4 + 1;
    if (grow(&d->dTape, &d->tape_cap, words)) return -1;
    HIPCHK(hipMemsetAsync(d->dTape, 0, words * 4, d->stream));
    if (len) HIPCHK(hipMemcpyAsync(d->dTape, tape, len, hipMemcpyHostToDevice, d->stream));
    HIPCHK(hipStreamSynchronize(d->stream));
    d->tape_len = len;
    /* A long tape (B1 in the 1e8s: 200 MB per prime range) runs as several launches.  Between two prac() calls only
     * the point A is live (PRAC_BEGIN sets B = C = A, ecm.c:603-608), and that is what every stage-1 kernel stores at
     * exit and loads at entry, so a launch may start at any PRAC_BEGIN byte — the 2-power doublings are such bytes
     * too.  The kernels read the tape as words: cuts are taken at offsets that are multiples of 4.  GECM_TAPE_CHUNK
     * (bytes) overrides the 16 MB default (tests cut short tapes with it). */
    size_t chunk = (size_t)16 << 20;
    if (const char *e = getenv("GECM_TAPE_CHUNK")) { long v = atol(e); if (v >= 4) chunk = (size_t)v; }
    d->tape_cuts.clear();
    d->tape_cuts.push_back(0);
    for (size_t want = chunk; want < len; ) {
        size_t off = (want + 3) & ~(size_t)3;
        while (off < len && tape[off] != GECM_OP_PRAC_BEGIN) off += 4;
        if (off >= len) break;
        d->tape_cuts.push_back(off);
        want = off + chunk;
    }
    d->tape_cuts.push_back(len);
    return 0;
}

/* Lanes per curve for this batch (tools/lanes_bench.py).  One curve per lane runs in
 * rounds of 2 wavefronts on each SIMD (4 per CU): full = 128 curves x SIMDs.  It is the faster layout
 * (by ~3%) only when its last round is nearly full; whenever that round would leave SIMDs idle or
 * half-occupied, two lanes per curve — twice the wavefronts, each half as long — fills them:
 * 1.83x below a quarter of `full`, 1.05x at half, 1.26x at three quarters.
 * From 26 limbs up (> 640-bit N) the split layout is the faster one at every batch size (all three
 * points stay in registers instead of one being parked in LDS: +1.5% at 26 limbs, +4% at 30, +10% at 37;
 * equal at 23 — tools/lanes_sizes.py, interleaved runs). */
extern "C" int gecm_dev_auto_lanes(gecm_dev *d)
{
    /* a batch that cannot even put one two-lane wavefront on every SIMD: eight lanes per curve (X and Z on two
     * quads, the limbs of a residue spread over the quad, csrc/gecm_quad.hpp) — 1.5x the two-lane layout at 15
     * limbs, 2.2-2.4x at 30-37 limbs, up to 32 curves per CU; from 19 limbs up still 1.2-1.4x at 64 curves
     * per CU (tools/quad_check.py).  Generic moduli only. */
    /* smaller still — at most 4 wavefronts of 2 curves on every SIMD: 32 lanes per curve (X and Z on two DPP rows,
     * the limbs over the 16 lanes of a row, csrc/gecm_row.hpp), the layout that puts BASELINE configs[1]'s 4096
     * curves on every SIMD of the chip twice: 1.8x the eight-lane layout at 4096 curves (415 and 831 bits), 1.3x
     * at 1023 bits, 1.05x at 8192 curves, slower from there on (tools/row_check.py).  Below 10 limbs the
     * 16 lanes of a row are mostly padding and the eight-lane layout wins. */
    /* Above 8192 curves (measured at 15, 30 and 37 limbs, profiles/r02_layouts_mid_batches.txt): the 32-lane kernel's
     * time grows with the batch, the eight- and two-lane kernels' in steps (one more wavefront per SIMD), so the
     * 32-lane layout still wins where the others have just taken a step: one limb per lane (up to 15 limbs) up to 56
     * curves per CU (18.7k against 16.2k curves/s at 12,288 curves, 415 bits; the two-lane layout takes over at
     * 14.4k); more limbs per lane up to 30 curves per CU and from 32 to 50 (831 bits: 31.9k against 29.7k curves/s at
     * 12,288), the eight-lane layout at exactly one or two wavefronts per SIMD in between (8192 curves: 32.7k against
     * 30.6k). */
    if (d->wide) return 32;                           // the one layout it has
    if (!d->multi && !d->fform && d->rowc.sets && d->nl >= 10 && d->stride) {
        const size_t s = d->stride, cu = (size_t)d->cus;
        if (d->rowc.nq == 1 ? s <= cu * 56 : (s <= cu * 30 || (s > cu * 32 && s <= cu * 50))) return 32;
    }
    /* Below 10 limbs the 32-lane layout still has the shortest chain per curve (9 rows of 6 instructions): while the
     * batch leaves it at one wavefront per SIMD or less (8 curves per CU) it is latency that counts — 8 curves of a
     * 204-bit N at B1 = 3e6: 4.11 s against 7.15 s (eight lanes) and 8.42 s (two), tools/multirange_time.py. */
    if (!d->multi && !d->fform && d->rowc.sets && d->nl < 10 &&d->stride && d->stride <= (size_t)d->cus * 8) return 32;
    if (!d->multi && !d->fform && d->dModQ && d->stride && d->stride <= (size_t)d->cus * (d->nl >= 19 ? 64 : 32)) return 8;
    if (d->nl >= 26) return 2;
    const size_t full = (size_t)d->cus * 4 * 128;
    const size_t r = d->stride % full;
    return (r == 0 || r > full / 4 * 3) ? 1 : 2;
}

/* 32-lane kernel, how the scanned operand of a multiply reaches its row (csrc/gecm_row.hpp): DPP broadcasts, or
 * (true) ds_swizzle through the LDS crossbar.  Two or three limbs per lane: the DPP rows (operand limbs two per
 * v_mov_b64_dpp) beat the crossbar by 8-12 % at every batch size from 4096 to 16,384 curves
 * (profiles/r03/mid_batch_rows.txt); one limb per lane: DPP up to two wavefronts per SIMD (4096 curves: 262 against
 * 284 ms), the crossbar from there (6144: 363 against 373; equal from 8192 on, tools/row_check.py). */
static bool row_a_lds(const gecm_dev *d)
{
    return d->rowc.nq == 1 && d->stride > (size_t)d->cus * 16;
}

extern "C" int gecm_dev_last_lanes(gecm_dev *d) { return d->last_lanes; }
extern "C" const char *gecm_dev_last_kernel(gecm_dev *d) { return d->last_kernel.c_str(); }

extern "C" int gecm_dev_fform_generic_limbs(int nl)
{
    const auto *kt = kernels_for(nl);
    return kt ? kt->p1()->fform_generic_limbs : -1;
}

extern "C" void gecm_dev_set_fform(gecm_dev *d, int form) { if (d->wide) return; d->fform = form == 2 ? 2 : form > 0 ? 1 : form < 0 ? -1 : 0; }

/* ---- stage 1: one plan, made from the request, and one run of it over the cuts of the tape ----
 * The request: a batch of curves with the lanes per curve asked for (0 = gecm_dev_auto_lanes), or with multi_rows the
 * 32-lane layout on a multi-modulus batch of either packing (lanes is then not looked at); or a P-1 / P+1
 * batch (unit; method GECM_UNIT_PM1 / _PP1) with 1 or 16 lanes per residue (§22). */
struct s1_request {
    bool unit;           // a P-1 / P+1 batch, of `method`
    int method, lanes;
    bool multi_rows;
};
enum s1_kind {
    S1_TABLE,        // stage1 of the limb count's table: one, two or eight lanes per curve, every constants source
    S1_TABLE_UNIT,   // its stage1_unit: a residue per lane
    S1_ROW,          // 32 lanes per curve (gecm_rowk.h) ...
    S1_ROW_WIDE,     // ... at the wide shapes
    S1_ROW_MULTI,    // ... on a multi-modulus batch
    S1_UNIT_ROW      // a residue per 16-lane row
};
struct s1_plan {
    s1_kind kind;
    const char *fn;      // the exported call, for the text of an error
    int lanes;           // per curve or residue
    bool a_lds, pp1;     // S1_ROW: operand limbs through the LDS crossbar (row_a_lds); the method is P+1
    bool canon_after;    // the kernel leaves lazy values and canon follows every launch
    char name[96];       // the kernel's name as rocprofv3 prints it
};

/* Every refusal of a stage-1 launch and every kernel name. */
static int s1_make_plan(gecm_dev *d, const s1_request &rq, s1_plan *p)
{
    auto refuse = [](const char *why) { g_err = why; return -2; };
    *p = {};                      // S1_TABLE, until a branch says otherwise
    p->fn = rq.unit ? "gecm_dev_stage1_unit" : rq.multi_rows ? "gecm_dev_stage1_multi_rows" : "gecm_dev_stage1";
    const char *entry = rq.unit ? "gecm_dev_stage1_unit" : "gecm_dev_stage1";
    if (rq.unit && ready(d, "gecm_dev_stage1_unit_lanes", NEEDS_TABLE)) return -2;
    if (rq.multi_rows && ready(d, p->fn, NEEDS_TABLE)) return -2;
    HIPCHK(hipSetDevice(d->device));
    if (ready(d, entry, NEEDS_BATCH)) return -2;
    if (!d->dTape) {
        g_err = std::string(entry) + ": no tape";
        return -2;
    }
    int lanes = rq.unit ? rq.lanes : rq.multi_rows ? 32 : rq.lanes ? rq.lanes : gecm_dev_auto_lanes(d);
    const char *base = nullptr;   // S1_TABLE, S1_TABLE_UNIT: the kernel is base<limbs>
    if (rq.unit) {
        if (rq.method != GECM_UNIT_PM1 && rq.method != GECM_UNIT_PP1) return refuse("gecm_dev_stage1_unit: the method must be P-1 or P+1");
        if (lanes != 1 && lanes != 16) return refuse("gecm_dev_stage1_unit: lanes per residue must be 1 or 16");
        if (lanes == 16 && !row_consts_ready(d, d->urowc))
            return refuse("gecm_dev_stage1_unit: the 16-lane kernel has no constants for this batch's moduli (gecm_dev_set_unit_rowconst)");
        if (d->multi && d->lane_packed && !d->k1->has_lane) return refuse("gecm_dev_stage1_unit: no per-lane kernels at this limb count");
        p->kind = lanes == 16 ? S1_UNIT_ROW : S1_TABLE_UNIT;
        p->pp1 = rq.method == GECM_UNIT_PP1;
        base = !d->multi ? "k_unit" : d->lane_packed ? "k_unit_lane" : "k_unit_multi";
    } else if (d->wide) {
        if (!d->rowc.sets) return refuse("gecm_dev_stage1: the wide context has no constants (gecm_dev_set_rowconst)");
        if (lanes != 32) return refuse("gecm_dev_stage1: a wide context runs with 32 lanes per curve (0 or 32)");
        p->kind = S1_ROW_WIDE;
    } else if (rq.multi_rows) {
        if (!gecm_dev_multi_rows_ready(d))
            return refuse("gecm_dev_stage1_multi_rows: the 32-lane kernel has no constants for this batch's moduli "
                          "(gecm_dev_set_multi_rowconst)");
        p->kind = S1_ROW_MULTI;
    } else if (d->multi && d->lane_packed) {
        if (rq.lanes > 1) return refuse("gecm_dev_stage1: a lane-packed multi-modulus batch runs with one lane per curve");
        lanes = 1;
        base = "k_stage1_lane";
    } else if (d->multi) {
        if (lanes != 1 && lanes != 2) return refuse("gecm_dev_stage1: a multi-modulus batch runs with 1 or 2 lanes per curve");
        base = lanes == 2 ? "k_stage1_pair_multi" : "k_stage1_multi";
    } else if (lanes == 32) {
        if (d->fform || !d->rowc.sets) return refuse("gecm_dev_stage1: no 32-lane kernel for this modulus");
        p->kind = S1_ROW;
        p->a_lds = row_a_lds(d);
    } else if (lanes == 8) {
        if (d->fform || !d->dModQ) return refuse("gecm_dev_stage1: no eight-lane kernel for this modulus");
        base = "k_stage1_quad";
    } else if (lanes == 1 || lanes == 2) {
        base = d->fform ? (lanes == 2 ? "k_stage1_pair_f" : "k_stage1_f") : lanes == 2 ? "k_stage1_pair" : "k_stage1";
    } else
        return refuse("gecm_dev_stage1: lanes per curve must be 0 (auto), 1, 2, 8 or 32");
    p->lanes = lanes;
    p->canon_after = p->kind == S1_UNIT_ROW || (!rq.unit && lanes >= 8 && p->kind != S1_ROW_WIDE);
    switch (p->kind) {
    case S1_ROW:
    case S1_ROW_WIDE:
        snprintf(p->name, sizeof p->name, "k_stage1_row<%d, %d, %s>", d->rowc.nq, d->rowc.rows, p->a_lds ? "true" : "false");
        break;
    case S1_ROW_MULTI: snprintf(p->name, sizeof p->name, "k_stage1_row_multi<%d, %d>", d->mrowc.nq, d->mrowc.rows); break;
    case S1_UNIT_ROW: snprintf(p->name, sizeof p->name, "k_unit_row<%d, %d>", d->urowc.nq, d->urowc.rows); break;
    case S1_TABLE:
        if (d->fform && !d->multi) {       // the special multiply (gecm_dev_set_fform)
            snprintf(p->name, sizeof p->name, "%s<%d, Mod%c<%d> >", base, d->nl, d->fform == 2 ? 'C' : d->fform > 0 ? 'F' : 'P', d->nl);
            break;
        }
        [[fallthrough]];
    case S1_TABLE_UNIT: snprintf(p->name, sizeof p->name, "%s<%d>", base, d->nl); break;
    }
    return 0;
}

/* The plan's kernel over every cut of the tape (gecm_dev_set_tape), asynchronous on the context's stream: an event per
 * launch (gecm_dev_stage1_progress), ev0 and ev1 around them all. */
static int s1_run_plan(gecm_dev *d, const s1_plan &p)
{
    d->last_lanes = p.lanes;
    d->last_kernel = p.name;
    gecm_modconst mc = modconst(d);
    HIPCHK(hipEventRecord(d->ev0, d->stream));
    d->cut_launches = d->tape_cuts.size() - 1;
    while (d->cut_events.size() < d->cut_launches) {
        hipEvent_t e;
        HIPCHK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
        d->cut_events.push_back(e);
    }
    for (size_t cut = 0; cut + 1 < d->tape_cuts.size(); cut++) {
        const uint32_t *tp = d->dTape + d->tape_cuts[cut] / 4;
        const uint32_t tl = (uint32_t)(d->tape_cuts[cut + 1] - d->tape_cuts[cut]);
        int unbuilt = 0;     // a row launcher's answer where the shape is not built
        switch (p.kind) {
        case S1_TABLE: d->k1->stage1(d->stream, &mc, tp, tl, d->dX, d->dZ, d->dS, d->stride, d->dModQ, p.lanes, d->fform); break;
        case S1_TABLE_UNIT: d->k1->stage1_unit(d->stream, &mc, tp, tl, d->dX, d->dZ, d->stride, p.pp1); break;
        case S1_ROW:
            unbuilt = gecm_launch_stage1_row(d->stream, d->rowc.nq, d->rowc.rows, tp, tl, d->dX, d->dZ, d->dS, d->stride,
                                             (uint32_t)d->nl, d->rowc.d, d->mod.rho, p.a_lds);
            break;
        case S1_ROW_WIDE:
            // nothing canonicalises between the launches or after them: the exit value of a launch is inside the contract
            // of the next one's entry multiply, and the host reduces what it downloads
            unbuilt = gecm_launch_stage1_row_wide(d->stream, d->rowc.rows, tp, tl, d->dX, d->dZ, d->dS, d->stride, (uint32_t)d->nl,
                                                  d->rowc.d, d->mod.rho);
            break;
        case S1_ROW_MULTI:
            unbuilt = gecm_launch_stage1_row_multi(d->stream, d->mrowc.nq, d->mrowc.rows, tp, tl, d->dX, d->dZ, d->dS, d->stride,
                                                   (uint32_t)d->nl, d->mrowc.d, mc.curve_group, mc.block_group);
            break;
        case S1_UNIT_ROW:
            unbuilt = gecm_launch_unit_row(d->stream, d->urowc.nq, d->urowc.rows, tp, tl, d->dX, d->stride, (uint32_t)d->nl, p.pp1,
                                           d->urowc.d, mc.curve_group, mc.block_group);
            break;
        }
        if (unbuilt) {
            g_err = std::string(p.fn) + ": no " + (p.kind == S1_UNIT_ROW ? "16" : "32") + "-lane kernel for this limb count";
            return -2;
        }
        if (p.canon_after) d->k1->canon(d->stream, &mc, d->dX, d->dZ, d->stride);
        HIPCHK(hipEventRecord(d->cut_events[cut], d->stream));
    }
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(d->ev1, d->stream));
    d->timed = true;
    return 0;
}

static int stage1_any(gecm_dev *d, const s1_request &rq)
{
    s1_plan p;
    if (const int rc = s1_make_plan(d, rq, &p)) return rc;
    return s1_run_plan(d, p);
}

extern "C" int gecm_dev_stage1(gecm_dev *d, int lanes_per_curve) { return stage1_any(d, {false, 0, lanes_per_curve, false}); }
extern "C" int gecm_dev_stage1_multi_rows(gecm_dev *d) { return stage1_any(d, {false, 0, 0, true}); }
extern "C" int gecm_dev_stage1_unit_lanes(gecm_dev *d, int method, int lanes) { return stage1_any(d, {true, method, lanes, false}); }

/* launches of the last gecm_dev_stage1 that have finished / that it made (a long tape runs as several) */
extern "C" int gecm_dev_stage1_progress(gecm_dev *d, uint32_t *done, uint32_t *total)
{
    uint32_t n = 0;
    for (size_t i = 0; i < d->cut_launches; i++) {
        if (hipEventQuery(d->cut_events[i]) != hipSuccess) break;    // in order on one stream
        n++;
    }
    (void)hipGetLastError();
    if (done) *done = n;
    if (total) *total = (uint32_t)d->cut_launches;
    return 0;
}

extern "C" int gecm_dev_sync(gecm_dev *d)
{
    HIPCHK(hipSetDevice(d->device));
    HIPCHK(hipStreamSynchronize(d->stream));
    if (d->timed) {
        HIPCHK(hipEventElapsedTime(&d->last_ms, d->ev0, d->ev1));
        d->timed = false;
    }
    return 0;
}

extern "C" float gecm_dev_last_kernel_ms(gecm_dev *d) { return d->last_ms; }

extern "C" int gecm_dev_download_mont(gecm_dev *d, uint32_t *X, uint32_t *Z)
{
    if (ready(d, "gecm_dev_download_mont", NEEDS_TABLE)) return -2;
    HIPCHK(hipSetDevice(d->device));
    if (download_soa(d, X, d->dX)) return -1;
    if (download_soa(d, Z, d->dZ)) return -1;
    HIPCHK(hipStreamSynchronize(d->stream));
    return 0;
}

extern "C" int gecm_dev_download_raw(gecm_dev *d, uint32_t *X, uint32_t *Z)
{
    HIPCHK(hipSetDevice(d->device));
    if (!d->stride) {
        g_err = "gecm_dev_download_raw: no batch";
        return -2;
    }
    if (download_soa(d, X, d->dX)) return -1;
    if (download_soa(d, Z, d->dZ)) return -1;
    HIPCHK(hipStreamSynchronize(d->stream));
    return 0;
}

extern "C" int gecm_dev_download_plain(gecm_dev *d, uint32_t *x, uint32_t *z)
{
    if (ready(d, "gecm_dev_download_plain", NEEDS_TABLE | NEEDS_BATCH)) return -2;
    HIPCHK(hipSetDevice(d->device));
    gecm_modconst mc = modconst(d);
    d->k1->from_mont(d->stream, &mc, d->dX, d->dZ, d->dT0, d->dT1, d->stride);
    HIPCHK(hipGetLastError());
    if (download_soa(d, x, d->dT0)) return -1;
    if (download_soa(d, z, d->dT1)) return -1;
    HIPCHK(hipStreamSynchronize(d->stream));
    return 0;
}

extern "C" int gecm_dev_l0(gecm_dev *d, int op, const uint32_t *a, const uint32_t *b, uint32_t *c,
                           uint32_t *dd, size_t count, const uint32_t *fix)
{
    if (ready(d, "gecm_dev_l0", NEEDS_TABLE)) return -2;
    HIPCHK(hipSetDevice(d->device));
    if (d->multi) {
        g_err = "gecm_dev_l0: not available on a multi-modulus context";
        return -2;
    }
    if (gecm_dev_resize(d, count)) return -1;
    // reuse the state buffers: X<-a, Z<-b, outputs T0, T1
    if (upload_soa(d, d->dX, a)) return -1;
    if (upload_soa(d, d->dZ, b ? b : a)) return -1;
    gecm_modconst mc = modconst(d);
    d->k1->l0(d->stream, &mc, op, d->dX, d->dZ, d->dT0, d->dT1, d->stride, fix ? fix : d->mod.one);
    HIPCHK(hipGetLastError());
    if (download_soa(d, c, d->dT0)) return -1;
    if (op == GECM_L0_ADDSUB && dd)
        if (download_soa(d, dd, d->dT1)) return -1;
    HIPCHK(hipStreamSynchronize(d->stream));
    return 0;
}

extern "C" int gecm_dev_l0_inv(gecm_dev *d, const uint32_t *a, uint32_t *inv, uint32_t *g, size_t count, const uint32_t *fix)
{
    if (ready(d, "gecm_dev_l0_inv", NEEDS_TABLE)) return -2;
    HIPCHK(hipSetDevice(d->device));
    if (d->multi || !d->mod.r3 || !fix) {
        g_err = "gecm_dev_l0_inv: needs a single-modulus context opened with its inversion constants (r3)";
        return -2;
    }
    if (gecm_dev_resize(d, count)) return -1;
    // as gecm_dev_l0: X<-a, outputs T0 (inverse), T1 (gcd); the padding lanes invert 0
    if (upload_soa(d, d->dX, a)) return -1;
    gecm_modconst mc = modconst(d);
    d->k1->l0_inv(d->stream, &mc, d->dX, d->dT0, d->dT1, d->stride, fix);
    HIPCHK(hipGetLastError());
    if (download_soa(d, inv, d->dT0)) return -1;
    if (download_soa(d, g, d->dT1)) return -1;
    HIPCHK(hipStreamSynchronize(d->stream));
    return 0;
}

// The raw operator works in planes of its own, freed when it returns: the batch of the context, which on a lane-packed
// context names the modulus of every position, stays as it is.
struct raw_planes {
    uint32_t *p = nullptr;
    ~raw_planes() { (void)hipFree(p); }
};

extern "C" int gecm_dev_l0_raw(gecm_dev *d, int op, int special, const uint32_t *a, const uint32_t *b, uint32_t *r, size_t count)
{
    if (ready(d, "gecm_dev_l0_raw", NEEDS_TABLE)) return -2;
    HIPCHK(hipSetDevice(d->device));
    const bool known = op == GECM_L0_MUL || op == GECM_L0_SQR || op == GECM_L0_ADD || op == GECM_L0_SUB || op == GECM_L0_CONDSUB;
    if (!known || !a || !r || !count) {
        g_err = "gecm_dev_l0_raw: needs an operator (MUL, SQR, ADD, SUB, CONDSUB), operands and a result";
        return -2;
    }
    if (d->multi && (!d->have_groups || !d->lane_packed || special || count != d->ncurves)) {
        g_err = "gecm_dev_l0_raw: a multi-modulus context takes one residue per position of its lane-packed batch, generic "
                "multiply";
        return -2;
    }
    const int form = special ? d->fform : 0;
    if (form == 2 && d->nl - d->k1->fform_generic_limbs < 3) {
        g_err = "gecm_dev_l0_raw: no 2^k - c multiply at this limb count";
        return -2;
    }
    const size_t stride = d->multi ? d->stride : (count + 63) / 64 * 64, plane = stride * d->nl;
    raw_planes m;
    HIPCHK(hipMalloc(&m.p, 3 * plane * sizeof(uint32_t)));
    // A, B with zero padding lanes; B = A where the operator has one operand
    HIPCHK(hipMemsetAsync(m.p, 0, 2 * plane * sizeof(uint32_t), d->stream));
    const uint32_t *src[2] = {a, b ? b : a};
    for (int q = 0; q < 2; q++)
        HIPCHK(hipMemcpy2DAsync(m.p + q * plane, stride * 4, src[q], count * 4, count * 4, d->nl, hipMemcpyHostToDevice,
                                d->stream));
    gecm_modconst mc = modconst(d);
    d->k1->l0_raw(d->stream, &mc, op, form, m.p, m.p + plane, m.p + 2 * plane, stride);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpy2DAsync(r, count * 4, m.p + 2 * plane, stride * 4, count * 4, d->nl, hipMemcpyDeviceToHost, d->stream));
    HIPCHK(hipStreamSynchronize(d->stream));
    return 0;
}

// ---------------------------------------------------------------- multi-modulus batches
extern "C" int gecm_dev_lane_packing_built(int nl)
{
    const auto *kt = kernels_for(nl);
    return kt ? kt->p1()->has_lane : 0;
}

extern "C" int gecm_dev_set_groups(gecm_dev *d, uint32_t ngroups, const gecm_devmod *mods, const uint32_t *block_group,
                                   const uint32_t *curve_group)
{
    if (ready(d, "gecm_dev_set_groups", NEEDS_TABLE)) return -2;
    HIPCHK(hipSetDevice(d->device));
    const size_t blocks = d->stride / 64, gb = d->k1->group_bytes;
    if (!d->multi || !ngroups || !blocks || !mods || (!block_group && !curve_group)) {
        g_err = "gecm_dev_set_groups: not a multi-modulus context, or no moduli or curves";
        return -2;
    }
    if (curve_group && !d->k1->has_lane) {
        g_err = "gecm_dev_set_groups: the per-lane kernels are not built for this limb count";
        return -2;
    }
    // the table the kernels of this batch read: a modulus per curve position, or one per 64-curve block
    const uint32_t *table = curve_group ? curve_group : block_group;
    for (size_t p = 0, entries = curve_group ? d->stride : blocks; p < entries; p++)
        if (table[p] >= ngroups) {
            g_err = std::string("gecm_dev_set_groups: ") + (curve_group ? "position " : "block ") + std::to_string(p) +
                    " names modulus " + std::to_string(table[p]);
            return -2;
        }
    std::vector<unsigned char> packed(gb * ngroups);
    for (uint32_t g = 0; g < ngroups; g++) {
        if (!mods[g].r3) {
            g_err = "gecm_dev_set_groups: modulus " + std::to_string(g) + " has no inversion constants (r3)";
            return -2;
        }
        d->k1->pack_group(&mods[g], packed.data() + g * gb);
    }
    if (grow(&d->dGroups, &d->groups_cap, packed.size()) || grow(&d->dBlockGroup, &d->blocks_cap, blocks) ||
        (curve_group && grow(&d->dCurveGroup, &d->curve_group_cap, d->stride)))
        return -1;
    // synchronous: the host arrays may go away when this returns, and no launch may see half of them
    HIPCHK(hipMemcpyAsync(d->dGroups, packed.data(), packed.size(), hipMemcpyHostToDevice, d->stream));
    if (curve_group) {       // the block table is not read, and defined
        HIPCHK(hipMemsetAsync(d->dBlockGroup, 0, blocks * sizeof(uint32_t), d->stream));
        HIPCHK(hipMemcpyAsync(d->dCurveGroup, curve_group, d->stride * sizeof(uint32_t), hipMemcpyHostToDevice, d->stream));
    } else
        HIPCHK(hipMemcpyAsync(d->dBlockGroup, block_group, blocks * sizeof(uint32_t), hipMemcpyHostToDevice, d->stream));
    HIPCHK(hipStreamSynchronize(d->stream));
    d->have_groups = true;
    d->ngroups = ngroups;
    d->lane_packed = curve_group != nullptr;
    return 0;
}

// ---------------------------------------------------------------- stage 2
/* Sub-sequences per curve for the stage-2 table build and giant steps: those are one dependent chain per curve, so a
 * batch of a few thousand curves (a few dozen wavefronts) is split into K interleaved chains per curve until there
 * are 2 wavefronts per SIMD (csrc/gecm_stage2.hpp, s2_init_k / giant_chunk_k).  1 for batches that fill the chip.
 * GECM_S2_SUBSEQ=1..32 (a power of two) overrides, for measurements.  A multi-modulus context keeps K = 1, whatever
 * the batch and the environment say, until gecm_dev_set_s2_subseq opts it in; a K set there holds on every context. */
static uint32_t s2_slices_for(const gecm_dev *d, size_t stride);
static uint32_t s2_subseq_for(const gecm_dev *d, size_t stride);

/* Device bytes a batch of `curves` curves takes: the five stage-1 arrays, and with npb != 0 the stage-2 allocations of
 * gecm_dev_s2_init for a table of npb entries, chunks of G giant steps and a ring of ring_size (with the sub-sequence
 * and slice counts a batch of that size gets).  The same sums as the hipMallocs below. */
extern "C" uint64_t gecm_dev_batch_bytes(gecm_dev *d, size_t curves, uint32_t npb, uint32_t G, uint32_t ring_size)
{
    const size_t stride = (curves + 63) / 64 * 64;
    const uint64_t coord = (uint64_t)d->nl * stride * sizeof(uint32_t);
    if (d->wide) return npb ? 0 : 3 * coord;                  // X, Z, S; no stage 2
    uint64_t words = 5 + 1;                                   // X, Z, S, two scratch arrays; factor-scan gcds
    if (npb) {
        const uint64_t K = s2_subseq_for(d, stride), slices = s2_slices_for(d, stride);
        words += (uint64_t)npb + 3 * GECM_S2_BLK + 2 + slices + (K > 1 ? K + 1 : 1) + (2 * ((uint64_t)G + 2) + G + ring_size);
        if (K > 1) {
            const uint64_t Gs = G / K + 1;
            words += K * 3 * GECM_S2_BLK + K * (2 * (Gs + 2) + Gs) + 2;
        }
    }
    return words * coord;
}

extern "C" uint32_t gecm_dev_s2_subseq(gecm_dev *d) { return s2_subseq_for(d, d->stride); }

extern "C" int gecm_dev_set_s2_subseq(gecm_dev *d, int k)
{
    if (ready(d, "gecm_dev_set_s2_subseq", NEEDS_TABLE)) return -2;
    if (k != 0 && k != -1 && (k < 1 || k > 32 || (k & (k - 1)))) return -2;
    d->s2_subseq_set = k;
    return 0;
}

extern "C" uint32_t gecm_dev_s2_k_chunks(gecm_dev *d) { return d->s2_k_chunks; }

static uint32_t s2_subseq_for(const gecm_dev *d, size_t stride)
{
    // two wavefronts per SIMD is the target (4096 curves, B2 = 1e8: K = 1 1.14 s, 4 0.75 s, 16 and 32 0.64 s)
    const size_t waves = stride / 64, want = (size_t)d->cus * 4 * 2;
    uint32_t k = 1;
    if (d->s2_subseq_set > 0) return (uint32_t)d->s2_subseq_set;
    if (d->multi && d->s2_subseq_set == 0) return 1;    // multi-modulus contexts: sub-sequences only when asked for
    while (k < 32 && waves * (k * 2) <= want) k *= 2;
    if (const char *e = getenv("GECM_S2_SUBSEQ")) {
        const long v = strtol(e, nullptr, 10);
        if (v >= 1 && v <= 32 && (v & (v - 1)) == 0) k = (uint32_t)v;
    }
    return k;
}

static uint32_t s2_slices_for(const gecm_dev *d, size_t stride)
{
    const size_t waves = stride / 64, want = (size_t)d->cus * 4 * GECM_S2_WAVES_PER_SIMD;
    size_t p = waves ? (want + waves - 1) / waves : 1;
    uint32_t s = (uint32_t)(p < 1 ? 1 : p > GECM_S2_MAX_SLICES ? GECM_S2_MAX_SLICES : p);
    if (const char *e = getenv("GECM_S2_SLICES")) {      // measurement knob (tools/s2_small.py)
        const long v = strtol(e, nullptr, 10);
        if (v >= 1 && v <= GECM_S2_MAX_SLICES) s = (uint32_t)v;
    }
    return s;
}

extern "C" uint32_t gecm_dev_s2_fail_planes(gecm_dev *d) { return d->s2_K > 1 ? d->s2_K + 1 : 1; }

/* method: 0 for a batch of curves, else GECM_UNIT_PM1 / GECM_UNIT_PP1.  Allocation, slices and the K
 * choice are the same for both; a method batch leaves the block scratch and the Z halves of Pd untouched. */
static int unit_method_ok(const gecm_dev *d, const char *fn, int method)
{
    if (method != GECM_UNIT_PM1 && method != GECM_UNIT_PP1) {
        g_err = std::string(fn) + ": the method must be P-1 or P+1";
        return -2;
    }
    if (d->multi && d->lane_packed && !d->k1->has_lane) {
        g_err = std::string(fn) + ": no per-lane kernels at this limb count";
        return -2;
    }
    return 0;
}

static int s2_init_any(gecm_dev *d, int method, const uint32_t *keep, size_t keep_words, uint32_t umax, uint32_t D,
                       uint32_t npb, uint32_t G, uint32_t ring_size, const uint32_t *tgt, const uint32_t *tgt_off, uint32_t K)
{
    if (ready(d, "gecm_dev_s2_init", NEEDS_TABLE | NEEDS_R3)) return -2;
    HIPCHK(hipSetDevice(d->device));
    const size_t coord = (size_t)d->nl * d->stride * sizeof(uint32_t);
    if (K < 1 || K > 32 || (K & (K - 1)) || (K > 1 && (!tgt || !tgt_off))) {
        g_err = "gecm_dev_s2_init: bad number of sub-sequences";
        return -2;
    }
    if (d->s2_npb != npb || d->s2_G != G || d->s2_ring != ring_size || d->s2_stride != d->stride || d->s2_K != K) {
        free_s2(d);
        d->s2_K = K;
        HIPCHK(hipMalloc(&d->dPbX, coord * npb));
        HIPCHK(hipMalloc(&d->dBlk, coord * 3 * GECM_S2_BLK));    // bx, bz, bp: S2_BLK entries each
        HIPCHK(hipMalloc(&d->dPd, coord * 2));
        // The pair walk is a product, so each run of pairs is walked in `slices` parts (one more grid dimension, one
        // accumulator each; slice 0 is the accumulator everyone else sees) until the launch has GECM_S2_WAVES_PER_SIMD
        // wavefronts for every SIMD.  Two per SIMD is what it takes to issue a multiply-add every 4.7 cycles, but the
        // walk also waits for table rows, and its 160 registers let three wavefronts share a SIMD: the full batch
        // (2048 wavefronts) went from 8.26 s to 7.68 s per 1e8 range with 4 slices, 7.57 s with 8; 32,768 curves from
        // 2.04 s (8 slices) to 1.96 s (32); 4096 curves from 0.380 s (32) to 0.371 s (64)
        // (profiles/r02_stage2_slices.txt).
        d->s2_slices = s2_slices_for(d, d->stride);
        HIPCHK(hipMalloc(&d->dAcc, coord * d->s2_slices));
        HIPCHK(hipMalloc(&d->dFail, coord * (K > 1 ? K + 1 : 1)));       // plane 0 + one per sub-sequence
        if (K > 1) {
            const size_t Gs = G / K + 1;
            HIPCHK(hipMalloc(&d->dKBlk, coord * K * 3 * GECM_S2_BLK));    // kbx, kbz, kbp per (curve block, r)
            HIPCHK(hipMalloc(&d->dKPa, coord * K * (2 * (Gs + 2) + Gs)));  // kgx, kgz (Gs+2 entries), kgp (Gs)
            HIPCHK(hipMalloc(&d->dPdK, coord * 2));
        }
        // giant steps: gx, gz (G+2 entries each), gp (G), ring (ring_size)
        HIPCHK(hipMalloc(&d->dPa, coord * (2 * ((size_t)G + 2) + (size_t)G + (size_t)ring_size)));
        d->s2_npb = npb; d->s2_G = G; d->s2_ring = ring_size; d->s2_stride = d->stride;
    }
    if (grow(&d->dKeep, &d->keep_cap, keep_words)) return -1;
    HIPCHK(hipMemcpyAsync(d->dKeep, keep, keep_words * 4, hipMemcpyHostToDevice, d->stream));
    if (K > 1) {
        const size_t tw = (size_t)tgt_off[K] + (K + 1);                 // target lists, then the K + 1 offsets
        if (grow(&d->dTgt, &d->tgt_cap, tw)) return -1;
        HIPCHK(hipMemcpyAsync(d->dTgt, tgt, (size_t)tgt_off[K] * 4, hipMemcpyHostToDevice, d->stream));
        HIPCHK(hipMemcpyAsync(d->dTgt + tgt_off[K], tgt_off, (K + 1) * 4, hipMemcpyHostToDevice, d->stream));
    }
    HIPCHK(hipMemsetAsync(d->dFail, 0, coord * (K > 1 ? K + 1 : 1), d->stream));
    HIPCHK(hipMemsetAsync(d->dPbX, 0, coord, d->stream));        // entry 0 (unused) defined
    gecm_s2_init_launch L;
    S2InitArgs &a = L.a;
    a.X = d->dX; a.Z = d->dZ; a.S = d->dS;
    a.PbX = d->dPbX;
    a.bx = d->dBlk; a.bz = d->dBlk + (coord / 4) * GECM_S2_BLK; a.bp = d->dBlk + (coord / 4) * 2 * GECM_S2_BLK;
    a.PdX = d->dPd; a.PdZ = d->dPd + coord / 4;
    a.acc = d->dAcc; a.fail = d->dFail; a.keep = d->dKeep;
    a.umax = umax; a.D = D; a.npb = npb; a.stride = d->stride;
    a.K = K;
    a.tgt = a.tgt_off = nullptr;
    a.kbx = a.kbz = a.kbp = a.PdKX = a.PdKZ = nullptr;
    if (K > 1) {
        const size_t kw = (coord / 4) * K * GECM_S2_BLK;
        a.tgt = d->dTgt; a.tgt_off = d->dTgt + tgt_off[K];
        a.kbx = d->dKBlk; a.kbz = d->dKBlk + kw; a.kbp = d->dKBlk + 2 * kw;
        a.PdKX = d->dPdK; a.PdKZ = d->dPdK + coord / 4;
    }
    L.slices = d->s2_slices;
    d->s2_k_chunks = 0;
    gecm_modconst mc = modconst(d);
    HIPCHK(hipEventRecord(d->ev0, d->stream));
    if (method) d->k2->s2_init_unit(d->stream, &mc, &L, method == GECM_UNIT_PM1);
    else d->k2->s2_init(d->stream, &mc, &L);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(d->ev1, d->stream));
    d->timed = true;
    return 0;
}

extern "C" int gecm_dev_s2_init(gecm_dev *d, const uint32_t *keep, size_t keep_words, uint32_t umax, uint32_t D,
                                uint32_t npb, uint32_t G, uint32_t ring_size, const uint32_t *tgt, const uint32_t *tgt_off,
                                uint32_t K)
{
    return s2_init_any(d, 0, keep, keep_words, umax, D, npb, G, ring_size, tgt, tgt_off, K);
}

extern "C" int gecm_dev_s2_init_unit(gecm_dev *d, int method, const uint32_t *keep, size_t keep_words, uint32_t umax,
                                     uint32_t D, uint32_t npb, uint32_t G, uint32_t ring_size, const uint32_t *tgt,
                                     const uint32_t *tgt_off, uint32_t K)
{
    if (unit_method_ok(d, "gecm_dev_s2_init_unit", method)) return -2;
    return s2_init_any(d, method, keep, keep_words, umax, D, npb, G, ring_size, tgt, tgt_off, K);
}

static int s2_pair_any(gecm_dev *d, int method, const uint32_t *steps, uint32_t nsteps, uint32_t D, uint32_t G,
                       uint32_t ring_size, uint64_t A0, uint64_t tape_id)
{
    if (ready(d, "gecm_dev_s2_pair", NEEDS_TABLE)) return -2;
    HIPCHK(hipSetDevice(d->device));
    if (!d->dPbX || d->s2_G != G || d->s2_ring != ring_size || (ring_size & (ring_size - 1))) {
        g_err = "gecm_dev_s2_pair: stage-2 init has not run (or chunk/ring size changed)";
        return -2;
    }
    const size_t coord = (size_t)d->nl * d->stride * sizeof(uint32_t);
    size_t words = (size_t)nsteps * 2 + 2;
    if (words > d->steps_cap) d->steps_id = 0;      // the kept copy goes with the array
    if (grow(&d->dSteps, &d->steps_cap, words)) return -1;
    // tape_id != 0 names a tape the host keeps from batch to batch: the device copy of the last one is kept too
    if (nsteps && !(tape_id && tape_id == d->steps_id && nsteps == d->steps_n))
        HIPCHK(hipMemcpyAsync(d->dSteps, steps, (size_t)nsteps * 8, hipMemcpyHostToDevice, d->stream));
    d->steps_id = tape_id;
    d->steps_n = nsteps;
    gecm_s2_pair_launch L;
    S2PairArgs &a = L.a;
    a.X = d->dX; a.Z = d->dZ; a.S = d->dS; a.PbX = d->dPbX; a.npb = (uint32_t)d->s2_npb;
    a.PdX = d->dPd; a.PdZ = d->dPd + coord / 4;
    const size_t cw = coord / 4;
    a.gx = d->dPa; a.gz = a.gx + cw * ((size_t)G + 2); a.gp = a.gz + cw * ((size_t)G + 2); a.ring = a.gp + cw * (size_t)G;
    a.acc = d->dAcc; a.fail = d->dFail; a.steps = d->dSteps; L.host_steps = steps;
    a.nsteps = nsteps; a.D = D; a.G = G; a.ring_size = ring_size; a.A0 = A0; a.stride = d->stride;
    L.slices = d->s2_slices;
    L.k_chunks = &d->s2_k_chunks;
    a.K = d->s2_K; a.Gs = (uint32_t)(G / d->s2_K + 1);
    a.kgx = a.kgz = a.kgp = nullptr; a.PdKX = a.PdKZ = nullptr;
    if (d->s2_K > 1) {
        const size_t kcw = cw * d->s2_K;
        a.kgx = d->dKPa; a.kgz = a.kgx + kcw * ((size_t)a.Gs + 2); a.kgp = a.kgz + kcw * ((size_t)a.Gs + 2);
        a.PdKX = d->dPdK; a.PdKZ = d->dPdK + cw;
    }
    gecm_modconst mc = modconst(d);
    HIPCHK(hipEventRecord(d->ev0, d->stream));
    if (method) d->k2->s2_pair_unit(d->stream, &mc, &L);
    else d->k2->s2_pair(d->stream, &mc, &L);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(d->ev1, d->stream));
    d->timed = true;
    return 0;
}

extern "C" int gecm_dev_s2_pair(gecm_dev *d, const uint32_t *steps, uint32_t nsteps, uint32_t D, uint32_t G,
                                uint32_t ring_size, uint64_t A0, uint64_t tape_id)
{
    return s2_pair_any(d, 0, steps, nsteps, D, G, ring_size, A0, tape_id);
}

extern "C" int gecm_dev_s2_pair_unit(gecm_dev *d, int method, const uint32_t *steps, uint32_t nsteps, uint32_t D, uint32_t G,
                                     uint32_t ring_size, uint64_t A0, uint64_t tape_id)
{
    if (unit_method_ok(d, "gecm_dev_s2_pair_unit", method)) return -2;
    return s2_pair_any(d, method, steps, nsteps, D, G, ring_size, A0, tape_id);
}

extern "C" int gecm_dev_s2_download(gecm_dev *d, uint32_t *acc, uint32_t *fail)
{
    if (ready(d, "gecm_dev_s2_download", NEEDS_TABLE)) return -2;
    HIPCHK(hipSetDevice(d->device));
    if (!d->dAcc) {
        g_err = "gecm_dev_s2_download: no stage-2 state";
        return -2;
    }
    if (download_soa(d, acc, d->dAcc)) return -1;
    if (fail) {          /* gecm_dev_s2_fail_planes() planes of [limb][ncurves] */
        const uint32_t planes = gecm_dev_s2_fail_planes(d);
        for (uint32_t p = 0; p < planes; p++)
            if (download_soa(d, fail + (size_t)p * d->nl * d->ncurves, d->dFail + (size_t)p * d->nl * d->stride)) return -1;
    }
    HIPCHK(hipStreamSynchronize(d->stream));
    return 0;
}

extern "C" int gecm_dev_gcd_scan(gecm_dev *d, int which, uint32_t *flags, uint32_t *g)
{
    if (ready(d, "gecm_dev_gcd_scan", NEEDS_TABLE)) return -2;
    HIPCHK(hipSetDevice(d->device));
    const uint32_t *src = which == 0 ? d->dZ : d->dAcc;
    if (!src) {
        g_err = "gecm_dev_gcd_scan: nothing to scan";
        return -2;
    }
    if (ready(d, "gecm_dev_gcd_scan", NEEDS_R3)) return -2;
    if (grow(&d->dFlags, &d->flags_cap, d->stride)) return -1;
    gecm_modconst mc = modconst(d);
    d->k1->gcd_scan(d->stream, &mc, src, d->dT0, d->dFlags, d->stride);
    HIPCHK(hipGetLastError());
    if (flags && d->ncurves)
        HIPCHK(hipMemcpyAsync(flags, d->dFlags, d->ncurves * 4, hipMemcpyDeviceToHost, d->stream));
    if (g && download_soa(d, g, d->dT0)) return -1;
    HIPCHK(hipStreamSynchronize(d->stream));
    return 0;
}

/* the factor scan of a P-1 / P+1 batch: gcd(x - off, N) for the residues in X, off = 1 or 2 */
extern "C" int gecm_dev_gcd_scan_off(gecm_dev *d, uint32_t off, uint32_t *flags, uint32_t *g)
{
    if (ready(d, "gecm_dev_gcd_scan_off", NEEDS_TABLE)) return -2;
    HIPCHK(hipSetDevice(d->device));
    if (off != 1 && off != 2) {
        g_err = "gecm_dev_gcd_scan_off: the offset is 1 or 2";
        return -2;
    }
    if (ready(d, "gecm_dev_gcd_scan_off", NEEDS_R3)) return -2;
    if (grow(&d->dFlags, &d->flags_cap, d->stride)) return -1;
    gecm_modconst mc = modconst(d);
    d->k1->gcd_scan_off(d->stream, &mc, d->dX, d->dT0, d->dFlags, d->stride, off);
    HIPCHK(hipGetLastError());
    if (flags && d->ncurves)
        HIPCHK(hipMemcpyAsync(flags, d->dFlags, d->ncurves * 4, hipMemcpyDeviceToHost, d->stream));
    if (g && download_soa(d, g, d->dT0)) return -1;
    HIPCHK(hipStreamSynchronize(d->stream));
    return 0;
}
