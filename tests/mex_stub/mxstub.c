/* A working stand-in for the subset of the MEX C API that mex/gsmcal_mex.c uses -- TEST INFRASTRUCTURE.
 *
 * mex.h beside it stays the strict declaration file; this file implements it, in the storage mode it is compiled for
 * (interleaved by default, split with -DGSMCAL_STUB_SPLIT), and adds the small harness (mxh_*) tests/mex_gateway.py drives
 * through ctypes.  One copy is compiled into every gateway object, with hidden visibility: only the mxh_* functions (and the
 * fake_* ones of fake_gsmcal.c) are exported, so an object binds its own stub and its own g_ctx whatever else the process holds.
 *
 * As strict as MATLAB where that finds bugs:
 *   - a typed accessor on an array of another class or complexity returns NULL (mxGetScalar of a non-numeric array is recorded);
 *   - mxCreateDoubleMatrix zero-fills; mxMalloc fills with 0xCD so that unwritten output shows;
 *   - every buffer the stub owns is followed by guard words, checked when the call ends;
 *   - mxFree of a pointer that is not live is recorded as a failure;
 *   - mxMalloc / mxCalloc memory the gateway did not free is released when the call returns (counted, not a failure);
 *   - mexErrMsgIdAndTxt longjmp()s to the harness; nothing allocated during the call survives it;
 *   - mexPrintf is captured per call; mexAtExit records the hook, mxh_run_atexit() runs it. */
#include <setjmp.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "mex.h"

#define MXH_API __attribute__((visibility("default")))
#define GUARD_WORDS 4
#define GUARD_PATTERN 0xA5C3F00DDEADBEEFull

enum { CLS_DOUBLE = 0, CLS_UINT8 = 1, CLS_LOGICAL = 2, CLS_CELL = 3 };
enum { K_ARRAY = 0, K_DATA = 1, K_MALLOC = 2 };

typedef struct block {          /* one buffer the stub owns: [block][payload][guard words] */
    struct block* next;
    size_t bytes;
    int kind;
    int in_call;                /* allocated while mexFunction ran */
    int kept;                   /* reachable from a returned plhs: survives the end of the call */
} block;

struct mxArray_tag {
    int cls, cplx;
    size_t m, n;
    void* re;                   /* interleaved mode: all the data; split mode: the real part (or the bytes / the cell pointers) */
    void* im;                   /* split mode, complex: the imaginary part */
};

static block* g_blocks = NULL;
static int g_in_call = 0;
static jmp_buf g_jmp;
static char g_err_id[256], g_err_msg[2048], g_printed[1 << 16], g_fail[4096];
static size_t g_printed_len = 0;
static int g_released = 0;
static void (*g_hooks[8])(void);
static int g_num_hooks = 0;
#define MAX_OUT 8
static mxArray* g_plhs[MAX_OUT];

static void fail(const char* fmt, ...) {
    size_t k = strlen(g_fail);
    va_list ap;
    va_start(ap, fmt);
    if (k < sizeof(g_fail) - 2) { vsnprintf(g_fail + k, sizeof(g_fail) - k - 2, fmt, ap); strcat(g_fail, "\n"); }
    va_end(ap);
}

static void* blk_alloc(size_t bytes, int kind, int fill) {
    block* b = (block*)malloc(sizeof(block) + bytes + GUARD_WORDS * sizeof(unsigned long long));
    unsigned long long g = GUARD_PATTERN;
    int i;
    if (!b) abort();
    b->bytes = bytes; b->kind = kind; b->in_call = g_in_call; b->kept = 0;
    b->next = g_blocks; g_blocks = b;
    memset(b + 1, fill, bytes);
    for (i = 0; i < GUARD_WORDS; ++i) memcpy((char*)(b + 1) + bytes + i * sizeof(g), &g, sizeof(g));
    return b + 1;
}
static int blk_guard_ok(const block* b) {
    unsigned long long g;
    int i;
    for (i = 0; i < GUARD_WORDS; ++i) {
        memcpy(&g, (const char*)(b + 1) + b->bytes + i * sizeof(g), sizeof(g));
        if (g != GUARD_PATTERN) return 0;
    }
    return 1;
}
static block* blk_find(const void* p) {
    block* b;
    for (b = g_blocks; b; b = b->next) if ((const void*)(b + 1) == p) return b;
    return NULL;
}
static void blk_free(block* b) {
    block** pp;
    for (pp = &g_blocks; *pp; pp = &(*pp)->next) if (*pp == b) { *pp = b->next; break; }
    if (!blk_guard_ok(b)) fail("guard words behind a %s of %lu bytes were overwritten", b->kind == K_MALLOC ? "mxMalloc block" : "mxArray buffer", (unsigned long)b->bytes);
    free(b);
}

static size_t elem_size(int cls) { return cls == CLS_DOUBLE ? sizeof(double) : cls == CLS_CELL ? sizeof(mxArray*) : 1; }

static mxArray* arr_new(int cls, int cplx, size_t m, size_t n) {
    mxArray* a = (mxArray*)blk_alloc(sizeof(mxArray), K_ARRAY, 0);
    size_t bytes = m * n * elem_size(cls);
    a->cls = cls; a->cplx = cplx; a->m = m; a->n = n;
#ifdef GSMCAL_STUB_SPLIT
    a->re = blk_alloc(bytes, K_DATA, 0);
    a->im = cplx ? blk_alloc(bytes, K_DATA, 0) : NULL;
#else
    a->re = blk_alloc(cplx ? 2 * bytes : bytes, K_DATA, 0);
    a->im = NULL;
#endif
    return a;
}
static void arr_free(mxArray* a) {
    block* b = blk_find(a);
    if (!b || b->kind != K_ARRAY) { fail("destroying something that is no live mxArray"); return; }
    if (a->cls == CLS_CELL) {
        size_t i;
        for (i = 0; i < a->m * a->n; ++i) if (((mxArray**)a->re)[i]) arr_free(((mxArray**)a->re)[i]);
    }
    if (a->im) blk_free(blk_find(a->im));
    blk_free(blk_find(a->re));
    blk_free(b);
}
static void arr_keep(mxArray* a) {
    block* b = blk_find(a);
    if (!b || b->kind != K_ARRAY) { fail("an output is no live mxArray"); return; }
    b->kept = 1;
    blk_find(a->re)->kept = 1;
    if (a->im) blk_find(a->im)->kept = 1;
    if (a->cls == CLS_CELL) {
        size_t i;
        for (i = 0; i < a->m * a->n; ++i) if (((mxArray**)a->re)[i]) arr_keep(((mxArray**)a->re)[i]);
    }
}

/* ---- the API of mex.h ----------------------------------------------------------------------------------------------- */
size_t mxGetM(const mxArray* a) { return a->m; }
size_t mxGetN(const mxArray* a) { return a->n; }
size_t mxGetNumberOfElements(const mxArray* a) { return a->m * a->n; }
int mxIsComplex(const mxArray* a) { return a->cplx; }
int mxIsUint8(const mxArray* a) { return a->cls == CLS_UINT8; }
#ifdef MATLAB_MEX_FILE
int mxIsDouble(const mxArray* a) { return a->cls == CLS_DOUBLE; }
#endif
double mxGetScalar(const mxArray* a) {
    if (a->cls == CLS_CELL || a->m * a->n == 0) { fail("mxGetScalar of a cell or an empty array"); return 0.0; }
    if (a->cls == CLS_DOUBLE) return ((const double*)a->re)[0];
    return (double)((const unsigned char*)a->re)[0];
}
#ifdef GSMCAL_STUB_SPLIT
double* mxGetPr(const mxArray* a) { return a->cls == CLS_DOUBLE ? (double*)a->re : NULL; }
double* mxGetPi(const mxArray* a) { return a->cls == CLS_DOUBLE && a->cplx ? (double*)a->im : NULL; }
void* mxGetData(const mxArray* a) { return a->re; }
#else
double* mxGetDoubles(const mxArray* a) { return a->cls == CLS_DOUBLE && !a->cplx ? (double*)a->re : NULL; }
mxComplexDouble* mxGetComplexDoubles(const mxArray* a) { return a->cls == CLS_DOUBLE && a->cplx ? (mxComplexDouble*)a->re : NULL; }
mxUint8* mxGetUint8s(const mxArray* a) { return a->cls == CLS_UINT8 && !a->cplx ? (mxUint8*)a->re : NULL; }
#endif
int mexPrintf(const char* fmt, ...) {
    va_list ap;
    int k;
    va_start(ap, fmt);
    k = vsnprintf(g_printed + g_printed_len, sizeof(g_printed) - g_printed_len, fmt, ap);
    va_end(ap);
    if (k > 0) g_printed_len += (size_t)k < sizeof(g_printed) - g_printed_len ? (size_t)k : sizeof(g_printed) - g_printed_len - 1;
    return k;
}
mxArray* mxCreateDoubleMatrix(mwSize m, mwSize n, mxComplexity flag) { return arr_new(CLS_DOUBLE, flag == mxCOMPLEX, m, n); }
mxArray* mxCreateDoubleScalar(double v) { mxArray* a = arr_new(CLS_DOUBLE, 0, 1, 1); ((double*)a->re)[0] = v; return a; }
mxArray* mxCreateLogicalScalar(mxLogical v) { mxArray* a = arr_new(CLS_LOGICAL, 0, 1, 1); ((unsigned char*)a->re)[0] = v ? 1 : 0; return a; }
mxArray* mxCreateCellMatrix(mwSize m, mwSize n) { return arr_new(CLS_CELL, 0, m, n); }
void mxSetCell(mxArray* cell, mwIndex i, mxArray* v) {
    if (cell->cls != CLS_CELL || i >= cell->m * cell->n) { fail("mxSetCell outside a cell array"); return; }
    ((mxArray**)cell->re)[i] = v;
}
void* mxMalloc(size_t n) { return blk_alloc(n, K_MALLOC, 0xCD); }
void* mxCalloc(size_t n, size_t s) { return blk_alloc(n * s, K_MALLOC, 0); }
void mxFree(void* p) {
    block* b;
    if (!p) return;
    b = blk_find(p);
    if (!b || b->kind != K_MALLOC) { fail("mxFree of a pointer that is not a live mxMalloc block"); return; }
    blk_free(b);
}
int mexAtExit(void (*fn)(void)) {
    if (g_num_hooks < 8) g_hooks[g_num_hooks++] = fn;
    return 0;
}
void mexErrMsgIdAndTxt(const char* id, const char* fmt, ...) {
    va_list ap;
    snprintf(g_err_id, sizeof(g_err_id), "%s", id);
    va_start(ap, fmt);
    vsnprintf(g_err_msg, sizeof(g_err_msg), fmt, ap);
    va_end(ap);
    if (!g_in_call) abort();                                    /* raised outside a call: nowhere to unwind to */
    longjmp(g_jmp, 1);
}

/* ---- the harness ------------------------------------------------------------------------------------------------------ */
MXH_API int mxh_interleaved(void) { return MX_HAS_INTERLEAVED_COMPLEX; }

/* An array from a caller's buffer, column-major; complex data is given interleaved (numpy's complex128) in either mode. */
MXH_API mxArray* mxh_create(int cls, int cplx, size_t m, size_t n, const void* data) {
    mxArray* a = arr_new(cls, cplx, m, n);
    size_t tot = m * n, i;
    if (!cplx) { memcpy(a->re, data, tot * elem_size(cls)); return a; }
#ifdef GSMCAL_STUB_SPLIT
    for (i = 0; i < tot; ++i) { ((double*)a->re)[i] = ((const double*)data)[2 * i]; ((double*)a->im)[i] = ((const double*)data)[2 * i + 1]; }
#else
    (void)i;
    memcpy(a->re, data, 2 * tot * sizeof(double));
#endif
    return a;
}
MXH_API void mxh_destroy(mxArray* a) { arr_free(a); }
MXH_API void mxh_info(const mxArray* a, int* cls, int* cplx, size_t* m, size_t* n) { *cls = a->cls; *cplx = a->cplx; *m = a->m; *n = a->n; }
/* data back out: doubles (interleaved when complex) or bytes */
MXH_API void mxh_read(const mxArray* a, void* dst) {
    size_t tot = a->m * a->n, i;
    if (!a->cplx) { memcpy(dst, a->re, tot * elem_size(a->cls)); return; }
#ifdef GSMCAL_STUB_SPLIT
    for (i = 0; i < tot; ++i) { ((double*)dst)[2 * i] = ((const double*)a->re)[i]; ((double*)dst)[2 * i + 1] = ((const double*)a->im)[i]; }
#else
    (void)i;
    memcpy(dst, a->re, 2 * tot * sizeof(double));
#endif
}
MXH_API mxArray* mxh_cell(const mxArray* a, size_t i) { return a->cls == CLS_CELL && i < a->m * a->n ? ((mxArray**)a->re)[i] : NULL; }
MXH_API mxArray* mxh_out(int i) { return i >= 0 && i < MAX_OUT ? g_plhs[i] : NULL; }
MXH_API const char* mxh_err_id(void) { return g_err_id; }
MXH_API const char* mxh_err_msg(void) { return g_err_msg; }
MXH_API const char* mxh_printed(void) { return g_printed; }
MXH_API const char* mxh_failures(void) { return g_fail; }
MXH_API int mxh_released(void) { return g_released; }           /* mxMalloc blocks the last call left for MATLAB to free */
MXH_API int mxh_live_blocks(void) { int k = 0; block* b; for (b = g_blocks; b; b = b->next) ++k; return k; }
MXH_API int mxh_num_hooks(void) { return g_num_hooks; }
MXH_API int mxh_run_atexit(void) {                               /* what MATLAB does when the MEX file is cleared */
    int i, k = g_num_hooks;
    for (i = 0; i < k; ++i) g_hooks[i]();
    g_num_hooks = 0;
    return k;
}

/* Calls mexFunction.  0: returned normally (outputs in mxh_out); 1: left through mexErrMsgIdAndTxt (no output survives).
 * The outputs of the call before are destroyed first. */
MXH_API int mxh_call(int nlhs, int nrhs, mxArray** prhs) {
    volatile int rc = 0;
    block *b, *next;
    int i;
    for (i = 0; i < MAX_OUT; ++i) if (g_plhs[i]) { arr_free(g_plhs[i]); g_plhs[i] = NULL; }
    g_err_id[0] = g_err_msg[0] = g_printed[0] = g_fail[0] = 0;
    g_printed_len = 0; g_released = 0;
    g_in_call = 1;
    if (setjmp(g_jmp) == 0) mexFunction(nlhs, g_plhs, nrhs, (const mxArray**)prhs);
    else rc = 1;
    g_in_call = 0;
    for (b = g_blocks; b; b = b->next) if (!blk_guard_ok(b)) fail("guard words behind a buffer of %lu bytes were overwritten", (unsigned long)b->bytes);
    if (rc) for (i = 0; i < MAX_OUT; ++i) g_plhs[i] = NULL;
    for (i = 0; i < MAX_OUT; ++i) if (g_plhs[i]) arr_keep(g_plhs[i]);
    for (b = g_blocks; b; b = next) {                           /* MATLAB's end of call: what is not an output goes */
        next = b->next;
        if (!b->in_call || b->kept) { b->in_call = 0; continue; }
        if (b->kind == K_MALLOC) ++g_released;
        blk_free(b);
    }
    return rc;
}
