/*
 * hea_oracle.c -- CPU fp64 ORACLE (plain C + OpenMP over the batch).  TEST INFRASTRUCTURE ONLY.
 *
 * Host twin of the device C ABI in include/quanonet_hea.h: same arguments with HOST
 * pointers and no workspace/stream.  It restates, gate by gate, the reference algorithm
 *   circuit   : core/quantum_circuits_tq.py:65-104  (== core/quantum_circuits_ms.py:127-226)
 *   read-out  : core/quantum_circuits_tq.py:106-127 (== core/quantum_circuits_ms.py:28-39)
 *   gradient  : adjoint differentiation, the scheme behind MindQuantum's
 *               get_expectation_with_grad (core/quantum_circuits_ms.py:229-233); batch-parallel
 *               over CPU threads like mqvector [upstream].
 * It deliberately applies every RX/RY/RZ/CNOT separately (no fusion) so that it is an
 * independent statement from the fused HIP kernels.  Pinned by tests/test_oracle_golden.py
 * against the numpy restatement and the reference's known answers K1-K8.
 *
 * Only tests/, __graft_entry__.smoke() and bench.py's cpu_baseline leg may load this library.
 *
 * One scalar type, `real`, carries all internal arithmetic: state, gate coefficients, cos / sin of the half angles, inner
 * products and accumulators.  The default is double (libhea_oracle.so, exports qhea_oracle_*).  -DQHEA_ORACLE_LONG_DOUBLE
 * builds the same source with long double (libhea_oracle_ld.so, exports qhea_oracle_ld_*): the reference that measures how
 * wrong the fp64 oracles themselves are.  Inputs are fp64 data either way (exact in the wider type), with an optional
 * second array of low parts for angles that no double holds (theta + pi/2 of the parameter-shift rule); every result v
 * comes back as hi = (double)v and, where the caller passes the array, lo = (double)(v - hi).
 */
#include <float.h>
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#ifdef _OPENMP
#include <omp.h>
#endif

#define MAXQ 14

#ifdef QHEA_ORACLE_LONG_DOUBLE
_Static_assert(LDBL_MANT_DIG >= 64, "the extended-precision oracle needs a long double of at least 64 mantissa bits");
typedef long double real;
#define R_COS cosl
#define R_SIN sinl
#define API(name) qhea_oracle_ld_##name
#else
typedef double real;
#define R_COS cos
#define R_SIN sin
#define API(name) qhea_oracle_##name
#endif

typedef struct { real re, im; } cplx;

/* a result array as the caller sees it: hi = (double)v, lo = (double)(v - hi) (lo may be absent) */
typedef struct { double* hi; double* lo; } outv;
static inline void put(outv o, long i, real v) {
    const double h = (double)v;
    o.hi[i] = h;
    if (o.lo) o.lo[i] = (double)(v - (real)h);
}
/* hi[i] + lo[i] in the internal type, as a fresh array (NULL for count 0 or on failure) */
static real* widen(const double* hi, const double* lo, long count) {
    if (count <= 0 || !hi) return NULL;
    real* r = (real*)malloc(sizeof(real) * (size_t)count);
    if (!r) return NULL;
    for (long i = 0; i < count; ++i) r[i] = lo ? (real)hi[i] + (real)lo[i] : (real)hi[i];
    return r;
}

static inline void rx(cplx* s, int n, int q, real th) {
    const real c = R_COS(0.5 * th), sn = R_SIN(0.5 * th);
    const long dim = 1L << n, m = 1L << q;
    for (long k = 0; k < dim; ++k) {
        if (k & m) continue;
        cplx a = s[k], b = s[k | m];
        /* [[c,-is],[-is,c]] */
        s[k].re = c * a.re + sn * b.im;     s[k].im = c * a.im - sn * b.re;
        s[k | m].re = c * b.re + sn * a.im; s[k | m].im = c * b.im - sn * a.re;
    }
}
static inline void ry(cplx* s, int n, int q, real th) {
    const real c = R_COS(0.5 * th), sn = R_SIN(0.5 * th);
    const long dim = 1L << n, m = 1L << q;
    for (long k = 0; k < dim; ++k) {
        if (k & m) continue;
        cplx a = s[k], b = s[k | m];
        /* [[c,-s],[s,c]] */
        s[k].re = c * a.re - sn * b.re;     s[k].im = c * a.im - sn * b.im;
        s[k | m].re = sn * a.re + c * b.re; s[k | m].im = sn * a.im + c * b.im;
    }
}
static inline void rz(cplx* s, int n, int q, real th) {
    const real c = R_COS(0.5 * th), sn = R_SIN(0.5 * th);
    const long dim = 1L << n, m = 1L << q;
    for (long k = 0; k < dim; ++k) {
        cplx a = s[k];
        if (k & m) { s[k].re = c * a.re - sn * a.im; s[k].im = c * a.im + sn * a.re; }   /* e^{+i th/2} */
        else       { s[k].re = c * a.re + sn * a.im; s[k].im = c * a.im - sn * a.re; }   /* e^{-i th/2} */
    }
}
static inline void cnot(cplx* s, int n, int control, int target) {
    const long dim = 1L << n, mc = 1L << control, mt = 1L << target;
    for (long k = 0; k < dim; ++k) {
        if ((k & mc) && !(k & mt)) { cplx t = s[k]; s[k] = s[k | mt]; s[k | mt] = t; }
    }
}
/* Im <lam| sigma_q |psi> */
static inline real im_inner(const cplx* lam, const cplx* psi, int n, int q, char pauli) {
    const long dim = 1L << n, m = 1L << q;
    real acc = 0.0;
    for (long k = 0; k < dim; ++k) {
        cplx l = lam[k], v;
        if (pauli == 'X') { v = psi[k ^ m]; }
        else if (pauli == 'Y') {
            cplx p = psi[k ^ m];
            if (k & m) { v.re = -p.im; v.im = p.re; }   /* (sigma_y psi)_1 = +i psi_0 */
            else       { v.re = p.im;  v.im = -p.re; }  /* (sigma_y psi)_0 = -i psi_1 */
        } else { v = psi[k]; if (k & m) { v.re = -v.re; v.im = -v.im; } }
        acc += l.re * v.im - l.im * v.re;               /* Im(conj(l) v) */
    }
    return acc;
}

static void run_forward(cplx* s, int n, int nb, const int32_t* enc, const int32_t* ld,
                        const real* xb, const real* w) {
    const long dim = 1L << n;
    memset(s, 0, sizeof(cplx) * dim);
    s[0].re = 1.0;
    long col = 0, blk = 0;
    for (int b = 0; b < nb; ++b) {
        for (int j = 0; j < enc[b]; ++j) rx(s, n, j % n, xb[col++]);
        for (int l = 0; l < ld[b]; ++l, ++blk) {
            const real* wb = w + blk * 3 * n;
            for (int i = 0; i < n; ++i) {
                ry(s, n, i, wb[0 * n + i]);
                rz(s, n, i, wb[1 * n + i]);
                ry(s, n, i, wb[2 * n + i]);
            }
            for (int i = 0; i < n; ++i) cnot(s, n, (i + 1) % n, i);
        }
    }
}

static inline real ham_k(long k, int n, real off, real co, const double* diag) {
    if (diag) return diag[k];
    return off + co * (real)(n - 2 * __builtin_popcountl((unsigned long)k));
}

/* hs = H s for H = off + co * sum_q P_q with P = X ('X') or Y ('Y'), written out Pauli by Pauli
 * (generate_simple_hamiltonian's `pauli`, core/quantum_circuits_ms.py:28-39).  Deliberately NOT the
 * basis-change trick the HIP kernels use, so the two stay independent statements. */
static void apply_pauli_ham(const cplx* s, cplx* hs, int n, real off, real co, int pauli) {
    const long dim = 1L << n;
    for (long k = 0; k < dim; ++k) {
        real re = off * s[k].re, im = off * s[k].im;
        for (int q = 0; q < n; ++q) {
            const long m = 1L << q;
            const cplx p = s[k ^ m];
            if (pauli == 1) { re += co * p.re; im += co * p.im; }
            else if (k & m) { re += co * -p.im; im += co * p.re; }     /* (sigma_y psi)_1 = +i psi_0 */
            else            { re += co * p.im;  im += co * -p.re; }    /* (sigma_y psi)_0 = -i psi_1 */
        }
        hs[k].re = re; hs[k].im = im;
    }
}

static int check(int n, int nb, const int32_t* enc, const int32_t* ld, long* E, long* blk) {
    if (n < 2 || n > MAXQ || nb < 0 || (nb > 0 && (!enc || !ld))) return -1;
    *E = 0; *blk = 0;
    for (int b = 0; b < nb; ++b) {
        if (enc[b] < 0 || ld[b] < 0) return -1;
        *E += enc[b]; *blk += ld[b];
    }
    return 0;
}

/* out[b] = <psi|H|psi> (and the final state) for internal-type angles x[B,E], w[blk*3*n] */
static void forward_core(int n, int nb, const int32_t* enc, const int32_t* ld, int64_t B, long E,
                         const real* x, const real* w, real off, real co,
                         const double* diag, int pauli, real* out, real* state_out) {
    const long dim = 1L << n;
#pragma omp parallel
    {
        cplx* s = (cplx*)malloc(sizeof(cplx) * dim);
        cplx* hs = (cplx*)malloc(sizeof(cplx) * dim);
#pragma omp for schedule(static)
        for (int64_t b = 0; b < B; ++b) {
            run_forward(s, n, nb, enc, ld, x + b * E, w);
            real acc = 0.0;
            if (pauli == 0) {
                for (long k = 0; k < dim; ++k)
                    acc += ham_k(k, n, off, co, diag) * (s[k].re * s[k].re + s[k].im * s[k].im);
            } else {
                apply_pauli_ham(s, hs, n, off, co, pauli);
                for (long k = 0; k < dim; ++k) acc += s[k].re * hs[k].re + s[k].im * hs[k].im;
            }
            out[b] = acc;
            if (state_out) memcpy(state_out + b * dim * 2, s, sizeof(cplx) * dim);
        }
        free(s); free(hs);
    }
}

/* adjoint differentiation: out[B] (may be absent), grad_x[B,E] and grad_w[P] in the internal type; 0 or -1 (no memory) */
static int backward_core(int n, int nb, const int32_t* enc, const int32_t* ld, int64_t B, long E, long blk,
                         const real* x, const real* w, real off, real co,
                         const double* diag, int pauli, const real* g,
                         real* out, real* grad_x, real* grad_w) {
    const long dim = 1L << n, P = blk * 3 * n;
    int nthreads = 1;
#ifdef _OPENMP
    nthreads = omp_get_max_threads();
#endif
    real* part = (real*)calloc((size_t)nthreads * (size_t)(P > 0 ? P : 1), sizeof(real));
    if (!part) return -1;
#pragma omp parallel
    {
        int tid = 0;
#ifdef _OPENMP
        tid = omp_get_thread_num();
#endif
        real* gw = part + (size_t)tid * (size_t)P;
        cplx* s = (cplx*)malloc(sizeof(cplx) * dim);
        cplx* lam = (cplx*)malloc(sizeof(cplx) * dim);
#pragma omp for schedule(static)
        for (int64_t b = 0; b < B; ++b) {
            const real* xb = x + b * E;
            real* gxb = grad_x + b * E;
            run_forward(s, n, nb, enc, ld, xb, w);
            real acc = 0.0;
            if (pauli == 0) {
                for (long k = 0; k < dim; ++k) {
                    const real h = ham_k(k, n, off, co, diag);
                    acc += h * (s[k].re * s[k].re + s[k].im * s[k].im);
                    lam[k].re = g[b] * h * s[k].re;
                    lam[k].im = g[b] * h * s[k].im;
                }
            } else {
                apply_pauli_ham(s, lam, n, off, co, pauli);
                for (long k = 0; k < dim; ++k) {
                    acc += s[k].re * lam[k].re + s[k].im * lam[k].im;
                    lam[k].re *= g[b]; lam[k].im *= g[b];
                }
            }
            if (out) out[b] = acc;
            long col = E, sub = blk;
            for (int bb = nb - 1; bb >= 0; --bb) {
                for (int l = ld[bb] - 1; l >= 0; --l) {
                    --sub;
                    const real* wb = w + sub * 3 * n;
                    real* gwb = gw + sub * 3 * n;
                    for (int i = n - 1; i >= 0; --i) { cnot(s, n, (i + 1) % n, i); cnot(lam, n, (i + 1) % n, i); }
                    for (int i = n - 1; i >= 0; --i) {
                        gwb[2 * n + i] += im_inner(lam, s, n, i, 'Y');
                        ry(s, n, i, -wb[2 * n + i]); ry(lam, n, i, -wb[2 * n + i]);
                        gwb[1 * n + i] += im_inner(lam, s, n, i, 'Z');
                        rz(s, n, i, -wb[1 * n + i]); rz(lam, n, i, -wb[1 * n + i]);
                        gwb[0 * n + i] += im_inner(lam, s, n, i, 'Y');
                        ry(s, n, i, -wb[0 * n + i]); ry(lam, n, i, -wb[0 * n + i]);
                    }
                }
                for (int j = enc[bb] - 1; j >= 0; --j) {
                    --col;
                    gxb[col] = im_inner(lam, s, n, j % n, 'X');
                    rx(s, n, j % n, -xb[col]); rx(lam, n, j % n, -xb[col]);
                }
            }
        }
        free(s); free(lam);
    }
    for (long p = 0; p < P; ++p) {
        real acc = 0.0;
        for (int t = 0; t < nthreads; ++t) acc += part[(size_t)t * (size_t)P + p];
        grad_w[p] = acc;
    }
    free(part);
    return 0;
}

static int forward_api(int n, int nb, const int32_t* enc, const int32_t* ld, int64_t B,
                       const double* x, const double* x_lo, const double* w, const double* w_lo, double off, double co,
                       const double* diag, int pauli, outv out, outv state_out) {
    long E, blk;
    if (check(n, nb, enc, ld, &E, &blk) || B < 0 || !out.hi || (B > 0 && E > 0 && !x) || (blk > 0 && !w))
        return -1;
    if (pauli < 0 || pauli > 2 || (pauli && diag)) return -1;
    const long S = state_out.hi ? B * (2L << n) : 0;
    real* xr = widen(x, x_lo, B * E);
    real* wr = widen(w, w_lo, blk * 3 * n);
    real* o = (real*)malloc(sizeof(real) * (size_t)(B > 0 ? B : 1));
    real* st = S > 0 ? (real*)malloc(sizeof(real) * (size_t)S) : NULL;
    int rc = ((B * E > 0 && !xr) || (blk > 0 && !wr) || !o || (S > 0 && !st)) ? -1 : 0;
    if (!rc) {
        forward_core(n, nb, enc, ld, B, E, xr, wr, off, co, diag, pauli, o, st);
        for (int64_t b = 0; b < B; ++b) put(out, b, o[b]);
        for (long i = 0; i < S; ++i) put(state_out, i, st[i]);
    }
    free(xr); free(wr); free(o); free(st);
    return rc;
}

static int backward_api(int n, int nb, const int32_t* enc, const int32_t* ld, int64_t B,
                        const double* x, const double* w, double off, double co,
                        const double* diag, int pauli, const double* g,
                        outv out, outv grad_x, outv grad_w) {
    long E, blk;
    if (check(n, nb, enc, ld, &E, &blk) || B < 0 || !g || !grad_x.hi || !grad_w.hi) return -1;
    if (pauli < 0 || pauli > 2 || (pauli && diag)) return -1;
    const long P = blk * 3 * n;
    real* xr = widen(x, NULL, B * E);
    real* wr = widen(w, NULL, P);
    real* gr = widen(g, NULL, B);
    real* o = (real*)malloc(sizeof(real) * (size_t)(B > 0 ? B : 1));
    real* gx = (real*)malloc(sizeof(real) * (size_t)(B * E > 0 ? B * E : 1));
    real* gw = (real*)malloc(sizeof(real) * (size_t)(P > 0 ? P : 1));
    int rc = ((B * E > 0 && !xr) || (P > 0 && !wr) || (B > 0 && !gr) || !o || !gx || !gw) ? -1 : 0;
    if (!rc) rc = backward_core(n, nb, enc, ld, B, E, blk, xr, wr, off, co, diag, pauli, gr, o, gx, gw);
    if (!rc) {
        if (out.hi) for (int64_t b = 0; b < B; ++b) put(out, b, o[b]);
        for (long i = 0; i < B * E; ++i) put(grad_x, i, gx[i]);
        for (long p = 0; p < P; ++p) put(grad_w, p, gw[p]);
    }
    free(xr); free(wr); free(gr); free(o); free(gx); free(gw);
    return rc;
}

#ifndef QHEA_ORACLE_LONG_DOUBLE
int qhea_oracle_forward(int n, int nb, const int32_t* enc, const int32_t* ld, int64_t B,
                        const double* x, const double* w, double off, double co,
                        const double* diag, int pauli, double* out, double* state_out) {
    return forward_api(n, nb, enc, ld, B, x, NULL, w, NULL, off, co, diag, pauli,
                       (outv){out, NULL}, (outv){state_out, NULL});
}

int qhea_oracle_backward(int n, int nb, const int32_t* enc, const int32_t* ld, int64_t B,
                         const double* x, const double* w, double off, double co,
                         const double* diag, int pauli, const double* g,
                         double* out, double* grad_x, double* grad_w) {
    return backward_api(n, nb, enc, ld, B, x, w, off, co, diag, pauli, g,
                        (outv){out, NULL}, (outv){grad_x, NULL}, (outv){grad_w, NULL});
}
#else
/* x_lo / w_lo: low parts of the angles (either may be NULL); state [B, 2^n, 2] */
int qhea_oracle_ld_forward(int n, int nb, const int32_t* enc, const int32_t* ld, int64_t B,
                           const double* x, const double* x_lo, const double* w, const double* w_lo, double off, double co,
                           const double* diag, int pauli, double* out_hi, double* out_lo,
                           double* state_hi, double* state_lo) {
    return forward_api(n, nb, enc, ld, B, x, x_lo, w, w_lo, off, co, diag, pauli,
                       (outv){out_hi, out_lo}, (outv){state_hi, state_lo});
}

int qhea_oracle_ld_backward(int n, int nb, const int32_t* enc, const int32_t* ld, int64_t B,
                            const double* x, const double* w, double off, double co,
                            const double* diag, int pauli, const double* g,
                            double* out_hi, double* out_lo, double* gx_hi, double* gx_lo, double* gw_hi, double* gw_lo) {
    return backward_api(n, nb, enc, ld, B, x, w, off, co, diag, pauli, g,
                        (outv){out_hi, out_lo}, (outv){gx_hi, gx_lo}, (outv){gw_hi, gw_lo});
}
#endif

/*
 * Model level, all of it in the internal type: the frequency layer x[b,k] = tin[b,k] * fw[k] + fb[k] on the tiled inputs
 * tin[B,E] (core/models_pt.py:38-41; the fixed-scale form :63-68 is fw[k] = scale_coeff, fb absent), out = circuit + bias,
 * the residuals against y, g = 2 resid / batch_total, the adjoint pass, and the chain rule into the frequency parameters
 * (d/d fw[k] = sum_b grad_x[b,k] tin[b,k], d/d fb[k] = sum_b grad_x[b,k]), the bias (sum_b g_b) and the sum of squared
 * residuals.  sse and grad_bias are (hi, lo) pairs; every other result a pair of arrays.
 */
int API(model_loss_grad)(int n, int nb, const int32_t* enc, const int32_t* ld, int64_t B,
                         const double* tin, const double* fw, const double* fb, const double* w,
                         double bias, const double* y, double batch_total,
                         double off, double co, const double* diag, int pauli,
                         double* sse, double* out_hi, double* out_lo, double* gw_hi, double* gw_lo,
                         double* gfw_hi, double* gfw_lo, double* gfb_hi, double* gfb_lo, double* grad_bias) {
    long E, blk;
    if (check(n, nb, enc, ld, &E, &blk) || B < 0 || !(batch_total > 0.0) || !sse || !out_hi || !gw_hi || !gfw_hi ||
        !gfb_hi || !grad_bias || (B > 0 && (!y || (E > 0 && (!tin || !fw)))) || (blk > 0 && !w))
        return -1;
    if (pauli < 0 || pauli > 2 || (pauli && diag)) return -1;
    const long P = blk * 3 * n;
    real* xr = (real*)malloc(sizeof(real) * (size_t)(B * E > 0 ? B * E : 1));
    real* wr = widen(w, NULL, P);
    real* o = (real*)malloc(sizeof(real) * (size_t)(B > 0 ? B : 1));
    real* g = (real*)malloc(sizeof(real) * (size_t)(B > 0 ? B : 1));
    real* gx = (real*)malloc(sizeof(real) * (size_t)(B * E > 0 ? B * E : 1));
    real* gw = (real*)malloc(sizeof(real) * (size_t)(P > 0 ? P : 1));
    int rc = (!xr || (P > 0 && !wr) || !o || !g || !gx || !gw) ? -1 : 0;
    if (!rc) {
        for (int64_t b = 0; b < B; ++b)
            for (long k = 0; k < E; ++k)
                xr[b * E + k] = (real)tin[b * E + k] * (real)fw[k] + (fb ? (real)fb[k] : (real)0.0);
        forward_core(n, nb, enc, ld, B, E, xr, wr, off, co, diag, pauli, o, NULL);
        real sq = 0.0, gb = 0.0;
        for (int64_t b = 0; b < B; ++b) {
            const real ob = o[b] + (real)bias, resid = ob - (real)y[b];
            put((outv){out_hi, out_lo}, b, ob);
            g[b] = (real)2.0 * resid / (real)batch_total;
            sq += resid * resid;
            gb += g[b];
        }
        put((outv){sse, sse + 1}, 0, sq);
        put((outv){grad_bias, grad_bias + 1}, 0, gb);
        rc = backward_core(n, nb, enc, ld, B, E, blk, xr, wr, off, co, diag, pauli, g, NULL, gx, gw);
    }
    if (!rc) {
        for (long p = 0; p < P; ++p) put((outv){gw_hi, gw_lo}, p, gw[p]);
        for (long k = 0; k < E; ++k) {
            real aw = 0.0, ab = 0.0;
            for (int64_t b = 0; b < B; ++b) { aw += gx[b * E + k] * (real)tin[b * E + k]; ab += gx[b * E + k]; }
            put((outv){gfw_hi, gfw_lo}, k, aw);
            put((outv){gfb_hi, gfb_lo}, k, ab);
        }
    }
    free(xr); free(wr); free(o); free(g); free(gx); free(gw);
    return rc;
}

int qhea_oracle_threads(void) {
#ifdef _OPENMP
    return omp_get_max_threads();
#else
    return 1;
#endif
}

/* number of OpenMP threads of the following calls (bench.py's 1-thread baseline leg); returns the previous maximum */
int qhea_oracle_set_threads(int n) {
#ifdef _OPENMP
    const int before = omp_get_max_threads();
    if (n > 0) omp_set_num_threads(n);
    return before;
#else
    (void)n;
    return 1;
#endif
}
