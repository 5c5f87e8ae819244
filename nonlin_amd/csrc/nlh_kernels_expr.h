// nlh_kernels_expr.h -- formula models (include/nonlin_hip.h: nlh_expr_*): the postfix program nlh_expr_compile makes of a
// user's expression, interpreted by residual and Jacobian kernels behind the launchers nlh_expr_device_fcn / _jac.
//
// THE ARITHMETIC IS PART OF THE INTERFACE; the table is in include/nonlin_hip.h and expr_run below is it, line for line:
// one IEEE operation per step (-ffp-contract=off), the device library's functions, tangents in forward mode with
// structural zeros (an absent operand is dropped, never multiplied).  No sum crosses a row.
//
// Shape (nlh_kernels_curve.h's): a thread per (point, row); the point's x staged in LDS; the row's variables, y and w
// loaded unconditionally (clamped index) ahead of the arithmetic; the Jacobian column-major with ld = m.  Two workgroup
// forms, the same bits: row (a workgroup per (point, 256 rows)) and flat (256 / m points per workgroup, short m).
//
// The program is uniform across the launch and travels by value in the kernel arguments (ExprProg, 2.6 KB): instruction
// fetch, dispatch, the stack pointer and every test of a dependency mask are scalar.  The stacks are indexed at run time, so
// they live in LDS as [slot][thread] columns (a wave's 64 lanes read 64 consecutive doubles: no bank conflict), depth
// slots deep -- the program's own depth, not the limit.  The Jacobian kernel carries the tangents of C consecutive columns
// per pass over the program, in C more such stacks, and recomputes the values in every pass: values do not depend on C, and
// a tangent only on its own column, so the bits are the table's for any C.  Which tangents exist is structural (the masks),
// hence uniform: nothing per thread records it.
#pragma once
#include "nlh_internal.h"
#include "nlh_kernels_place.h"
#include "nlh_kernels_specfun.h"
#include "nlh_kernels_specfun2.h"

struct ExprData {                      // what the kernels read of an nlh_expr_ctx
    int shared_t, m;
    long long tstride;                 // doubles between the variables' blocks of t
    const double *t, *y, *w;           // y, w may be null (model values: nlh_expr_eval_batch)
};

#define EXPR_OP(c)     ((int)((c) & 0xffu))
#define EXPR_ARG(c)    ((int)(int8_t)(((c) >> 8) & 0xffu))
#define EXPR_AROOT(c)  ((int)(((c) >> 16) & 0xffu))
#define EXPR_BROOT(c)  ((int)(((c) >> 24) & 0xffu))   // VOIGT, WHERE: the producer of the second operand

// The device library's erf, erfc and erfcx behind one call: inlined three times into the interpreter they cost it 70 VGPRs
// (and k_expr_fcn a wave per SIMD) whether or not a formula uses them.
__device__ static __noinline__ double expr_erf_family(int op, double a)
{
    return op == NLH_EXPR_ERF ? erf(a) : (op == NLH_EXPR_ERFC ? erfc(a) : erfcx(a));
}

// The device library's pow, atan2 and the log of POW's exponent partial behind one call (sel: NLH_EXPR_POW, NLH_EXPR_ATAN2,
// anything else log(a)), for the same reason: k_expr_fcn sits a few VGPRs under its occupancy step, so pow is
// not inlined a second and third time, log a second and atan2 a first.
__device__ static __noinline__ double expr_pow_family(int sel, double a, double b)
{
    return sel == NLH_EXPR_POW ? pow(a, b) : (sel == NLH_EXPR_ATAN2 ? atan2(a, b) : log(a));
}

// The functions of NLH_EXPR_J0 .. NLH_EXPR_LOG1P behind one call, value and g of the header's table returned by value (a
// pointer out-parameter costs every lane 16 bytes of scratch): the device library's j0, j1, lgamma, expm1, log1p, exp and
// the stated i0e, i1e and digamma (nlh_kernels_specfun2.h), each inlined once.  tan: the operand has a tangent in this
// pass (uniform); g is computed only then.  LOG1P's g is the divisor 1.0 + a.
struct ExprSf2 { double v, g; };
__device__ static __noinline__ ExprSf2 expr_sf2_family(int op, double a, bool tan)
{
    ExprSf2 r;
    r.g = 0.0;
    if (op <= NLH_EXPR_J1) {
        const double f0 = op == NLH_EXPR_J0 || tan ? j0(a) : 0.0, f1 = op == NLH_EXPR_J1 || tan ? j1(a) : 0.0;
        if (op == NLH_EXPR_J0) { r.v = f0; r.g = f1; }
        else { r.v = f1; if (tan) r.g = a == 0.0 ? 0.5 : f0 - f1 / a; }
    }
    else if (op <= NLH_EXPR_I1E) {
        const double f0 = op == NLH_EXPR_I0E || tan ? sf2_i0e(a) : 0.0, f1 = op == NLH_EXPR_I1E || tan ? sf2_i1e(a) : 0.0;
        if (op == NLH_EXPR_I0E) { r.v = f0; if (tan) { const double s = a < 0.0 ? -f0 : f0; r.g = f1 - s; } }
        else { r.v = f1; if (tan) { const double s = a < 0.0 ? -f1 : f1; r.g = a == 0.0 ? 0.5 : (f0 - s) - f1 / a; } }
    }
    else if (op == NLH_EXPR_LGAMMA) { r.v = lgamma(a); if (tan) r.g = sf2_digamma(a); }
    else if (op == NLH_EXPR_EXPM1) { r.v = expm1(a); if (tan) r.g = exp(a); }
    else { r.v = log1p(a); r.g = 1.0 + a; }
    return r;
}

// One pass over the program.  vs: this thread's column of the value stack (slot s at vs[s * 256]); ts: of the C tangent
// stacks (column c, slot s at ts[(c * depth + s) * 256]), columns j0 .. j0 + C - 1 (C = 0: values only).  Statement k of a
// formula with definitions leaves its root in slot k, where LOAD k reads it; nothing stores.  Returns the root's value; the
// root's tangents are left in the slot it ends in: slot 0 without definitions, slot ndef with them, which `slot` receives.
// KIND: what the program holds beyond the older instruction set -- EXPR_PLAIN nothing, EXPR_DEFS definitions, EXPR_SF2 an
// instruction of NLH_EXPR_J0 .. NLH_EXPR_LOG1P (and definitions or none: with ndef = 0 the frame costs nothing).  The
// launcher chooses; a lower kind is, instruction for instruction, the interpreter it was before the higher one existed --
// EXPR_PLAIN: no LOAD block, the result in slot 0; below EXPR_SF2: no block of the newer functions and no call of their
// family -- so the older formulas run the code they ran.
enum { EXPR_PLAIN = 0, EXPR_DEFS = 1, EXPR_SF2 = 2 };
template <bool TAN, int KIND>
__device__ static inline double expr_run(const ExprProg &P, const double *xq, const double (&tv)[NLH_EXPR_MAX_VARS], double *vs, double *ts,
                                         int j0, int C, int &slot)
{
    const int depth = P.depth;
    const uint32_t cm = !TAN ? 0u : (C >= 32 ? 0xffffffffu : (1u << C) - 1u);   // (values only: every tangent test folds away)
    int sp = 0;                                                   // slots in use (scalar)
#define V(s) vs[(s) * 256]
#define T(c, s) ts[((c) * depth + (s)) * 256]
    for (int pc = 0; pc < P.ninstr; ++pc) {
        const uint32_t code = P.code[pc];
        const int op = EXPR_OP(code), arg = EXPR_ARG(code);
        if (op <= NLH_EXPR_PARAM) {
            double v;
            if (op == NLH_EXPR_CONST) v = P.consts[arg];
            else if (op == NLH_EXPR_VAR) v = arg == 0 ? tv[0] : (arg == 1 ? tv[1] : (arg == 2 ? tv[2] : tv[3]));
            else {
                v = xq[arg];
                if (TAN && arg >= j0 && arg < j0 + C) T(arg - j0, sp) = 1.0;
            }
            V(sp) = v;
            ++sp;
            continue;
        }
        if (op >= NLH_EXPR_ADD && op <= NLH_EXPR_DIV) {           // binary: a below b
            const double a = V(sp - 2), b = V(sp - 1);
            const uint32_t ma = (P.mask[EXPR_AROOT(code)] >> j0) & cm, mb = (P.mask[pc - 1] >> j0) & cm;
            double v, q = 0.0;
            if (op == NLH_EXPR_ADD) v = a + b;
            else if (op == NLH_EXPR_SUB) v = a - b;
            else if (op == NLH_EXPR_MUL) v = a * b;
            else { q = a / b; v = q; }
            for (uint32_t mm = ma | mb; mm; mm &= mm - 1) {
                const int c = __builtin_ctz(mm);
                const bool ha = (ma >> c) & 1u, hb = (mb >> c) & 1u;
                const double da = ha ? T(c, sp - 2) : 0.0, db = hb ? T(c, sp - 1) : 0.0;
                double d;
                if (op == NLH_EXPR_ADD) d = ha && hb ? da + db : (ha ? da : db);
                else if (op == NLH_EXPR_SUB) d = ha && hb ? da - db : (ha ? da : -db);
                else if (op == NLH_EXPR_MUL) d = ha && hb ? da * b + a * db : (ha ? da * b : a * db);
                else d = ha && hb ? (da - q * db) / b : (ha ? da / b : -((q * db) / b));
                T(c, sp - 2) = d;
            }
            V(sp - 2) = v;
            --sp;
            continue;
        }
        if (op >= NLH_EXPR_VOIGT) {                               // the functions of several operands and LOAD, behind the one test VOIGT had:
                                                                  // a test more per instruction cost the older formulas 2 - 3 %
            if (op == NLH_EXPR_VOIGT) {                           // ternary: x below sigma below gamma; w(z) once per pass
                const double a = V(sp - 3), b = V(sp - 2), c3 = V(sp - 1);
                const uint32_t ma = (P.mask[EXPR_AROOT(code)] >> j0) & cm, mb = (P.mask[EXPR_BROOT(code)] >> j0) & cm,
                               mc = (P.mask[pc - 1] >> j0) & cm;
                double gx, gs, gg;
                const double v = voigt_eval(a, b, c3, &gx, &gs, &gg);
                for (uint32_t mm = ma | mb | mc; mm; mm &= mm - 1) {
                    const int c = __builtin_ctz(mm);
                    const bool ha = (ma >> c) & 1u, hb = (mb >> c) & 1u, hc = (mc >> c) & 1u;
                    double d = 0.0;
                    if (ha) d = gx * T(c, sp - 3);
                    if (hb) d = ha ? d + gs * T(c, sp - 2) : gs * T(c, sp - 2);
                    if (hc) d = ha || hb ? d + gg * T(c, sp - 1) : gg * T(c, sp - 1);
                    T(c, sp - 3) = d;
                }
                V(sp - 3) = v;
                sp -= 2;
                continue;
            }
            if (op == NLH_EXPR_WHERE) {                           // ternary: c below a below b; both branches were evaluated
                const bool s = V(sp - 3) >= 0.0;
                const uint32_t ma = (P.mask[EXPR_BROOT(code)] >> j0) & cm, mb = (P.mask[pc - 1] >> j0) & cm,
                               mc = (P.mask[EXPR_AROOT(code)] >> j0) & cm;
                for (uint32_t mm = ma | mb | mc; mm; mm &= mm - 1) {  // (c's tangent is overwritten unread)
                    const int c = __builtin_ctz(mm);
                    const double da = (ma >> c) & 1u ? T(c, sp - 2) : 0.0, db = (mb >> c) & 1u ? T(c, sp - 1) : 0.0;
                    T(c, sp - 3) = s ? da : db;
                }
                V(sp - 3) = s ? V(sp - 2) : V(sp - 1);
                sp -= 2;
                continue;
            }
            if (KIND >= EXPR_DEFS && op == NLH_EXPR_LOAD) {       // a use of definition arg: a copy of slot arg, the value and the
                                                                  // tangents its mask names; the slot itself stays
                for (uint32_t mm = (P.mask[pc] >> j0) & cm; mm; mm &= mm - 1) {
                    const int c = __builtin_ctz(mm);
                    T(c, sp) = T(c, arg);
                }
                V(sp) = V(arg);
                ++sp;
                continue;
            }
            if (KIND >= EXPR_SF2 && op >= NLH_EXPR_J0) {          // J0 .. LOG1P: unary, one call for the value and g
                const double a = V(sp - 1);
                const uint32_t ma = (P.mask[pc - 1] >> j0) & cm;
                const ExprSf2 f = expr_sf2_family(op, a, ma != 0u);
                for (uint32_t mm = ma; mm; mm &= mm - 1) {
                    const int c = __builtin_ctz(mm);
                    const double da = T(c, sp - 1);
                    T(c, sp - 1) = op == NLH_EXPR_LOG1P ? da / f.g : (op == NLH_EXPR_J0 ? -(f.g * da) : f.g * da);
                }
                V(sp - 1) = f.v;
                continue;
            }
            // POW, ATAN2, MIN, MAX: binary, a below b (ADD .. DIV keep the block they had)
            const double a = V(sp - 2), b = V(sp - 1);
            const uint32_t ma = (P.mask[EXPR_AROOT(code)] >> j0) & cm, mb = (P.mask[pc - 1] >> j0) & cm;
            double v, ga = 0.0, gb = 0.0;                         // POW: the partials; ATAN2: ga = den
            bool s = false;                                       // MIN, MAX: b is selected (per lane)
            if (op == NLH_EXPR_POW) {
                v = expr_pow_family(NLH_EXPR_POW, a, b);
                if (ma) ga = b * expr_pow_family(NLH_EXPR_POW, a, b - 1.0);
                if (mb) { const double l = expr_pow_family(NLH_EXPR_LOG, a, b); gb = v == 0.0 ? 0.0 : v * l; }
            }
            else if (op == NLH_EXPR_ATAN2) { v = expr_pow_family(NLH_EXPR_ATAN2, a, b); ga = a * a + b * b; }
            else { s = op == NLH_EXPR_MAX ? b > a : b < a; v = s ? b : a; }
            for (uint32_t mm = ma | mb; mm; mm &= mm - 1) {
                const int c = __builtin_ctz(mm);
                const bool ha = (ma >> c) & 1u, hb = (mb >> c) & 1u;
                const double da = ha ? T(c, sp - 2) : 0.0, db = hb ? T(c, sp - 1) : 0.0;
                double d;
                if (op == NLH_EXPR_POW) {
                    const double ta = da == 0.0 ? 0.0 : ga * da, tb = gb * db;
                    d = ha && hb ? ta + tb : (ha ? ta : tb);
                }
                else if (op == NLH_EXPR_ATAN2) d = ha && hb ? (b * da - a * db) / ga : (ha ? (b * da) / ga : -((a * db) / ga));
                else d = s ? db : da;                             // (an absent operand's tangent is the +0.0 above)
                T(c, sp - 2) = d;
            }
            V(sp - 2) = v;
            --sp;
            continue;
        }
        // unary: the operand is the instruction before
        const double a = V(sp - 1);
        const uint32_t ma = (P.mask[pc - 1] >> j0) & cm;
        double v, g = 0.0;                                        // the tangent is g * da (or the op's own form below)
        switch (op) {
        case NLH_EXPR_NEG: v = -a; break;
        case NLH_EXPR_IPOW: {
            const int k = arg < 0 ? -arg : arg;
            double u = a;
            v = a;
            for (int r = 1; r < k; ++r) { u = v; v = v * a; }
            g = (double)k * u;
            if (arg < 0) v = 1.0 / v;
            break;
        }
        case NLH_EXPR_POWC: {
            const double c = P.consts[arg];
            v = pow(a, c);
            if (ma) g = c * pow(a, c - 1.0);
            break;
        }
        case NLH_EXPR_EXP: v = exp(a); break;
        case NLH_EXPR_LOG: v = log(a); break;
        case NLH_EXPR_SQRT: v = sqrt(a); break;
        case NLH_EXPR_SIN: v = sin(a); if (ma) g = cos(a); break;
        case NLH_EXPR_COS: v = cos(a); if (ma) g = sin(a); break;
        case NLH_EXPR_TANH: v = tanh(a); break;
        case NLH_EXPR_ATAN: v = atan(a); break;
        case NLH_EXPR_ERF: v = expr_erf_family(op, a); if (ma) g = NLH_SF_C1 * exp(-(a * a)); break;
        case NLH_EXPR_ERFC: v = expr_erf_family(op, a); if (ma) g = NLH_SF_C1 * exp(-(a * a)); break;
        case NLH_EXPR_ERFCX: v = expr_erf_family(op, a); break;
        default: v = fabs(a); break;                              // NLH_EXPR_ABS
        }
        for (uint32_t mm = ma; mm; mm &= mm - 1) {
            const int c = __builtin_ctz(mm);
            const double da = T(c, sp - 1);
            double d;
            switch (op) {
            case NLH_EXPR_NEG: d = -da; break;
            case NLH_EXPR_IPOW: d = arg > 0 ? g * da : -((g * da) * (v * v)); break;
            case NLH_EXPR_POWC: d = g * da; break;
            case NLH_EXPR_EXP: d = v * da; break;
            case NLH_EXPR_LOG: d = da / a; break;
            case NLH_EXPR_SQRT: d = da / (2.0 * v); break;
            case NLH_EXPR_SIN: d = g * da; break;
            case NLH_EXPR_COS: d = -(g * da); break;
            case NLH_EXPR_TANH: d = (1.0 - v * v) * da; break;
            case NLH_EXPR_ATAN: d = da / (1.0 + a * a); break;
            case NLH_EXPR_ERF: d = g * da; break;
            case NLH_EXPR_ERFC: d = -(g * da); break;
            case NLH_EXPR_ERFCX: d = ((2.0 * a) * v - NLH_SF_C1) * da; break;
            default: d = a < 0.0 ? -da : da; break;
            }
            T(c, sp - 1) = d;
        }
        V(sp - 1) = v;
    }
    if (KIND >= EXPR_DEFS) { slot = sp - 1; return V(sp - 1); }
    return V(0);
#undef V
#undef T
}

// the row's variables, loaded whether or not the thread has a row (clamped index)
__device__ static inline void expr_load_vars(const ExprData &ed, int nvar, size_t at, int ic, double (&tv)[NLH_EXPR_MAX_VARS])
{
    const size_t o = ed.shared_t ? (size_t)ic : at;
#pragma unroll
    for (int v = 0; v < NLH_EXPR_MAX_VARS; ++v) tv[v] = ed.t[v < nvar ? o + (size_t)v * (size_t)ed.tstride : o];
}

template <bool FLAT, int KIND>
static __global__ void __launch_bounds__(256)
k_expr_fcn(const ExprProg P, ExprData ed, int n, int nblk, int ppw, int npoints, const int32_t *__restrict__ dprob,
           const double *__restrict__ X, double *__restrict__ F)
{
    extern __shared__ double lds[];                               // x of the workgroup's points, then the value stack
    int q, i;
    const double *xq;
    const bool on = place_staged<FLAT>(ed.m, n, nblk, ppw, npoints, X, lds, q, i, xq);
    const int qc = min(q, npoints - 1), ic = min(i, ed.m - 1);
    const int p = dprob ? dprob[qc] : qc;
    const size_t at = (size_t)p * ed.m + ic;
    double tv[NLH_EXPR_MAX_VARS];
    expr_load_vars(ed, P.nvar, at, ic, tv);
    const double y = ed.y ? ed.y[at] : 0.0;
    const double w = ed.w ? ed.w[at] : 1.0;
    if (!on) return;
    double *vs = lds + (FLAT ? ppw : 1) * n + threadIdx.x;
    int slot = 0;
    double r = expr_run<false, KIND>(P, xq, tv, vs, vs, 0, 0, slot);
    if (ed.y) r = r - y;
    if (ed.w) r = w * r;
    F[(size_t)q * ed.m + i] = r;
}

template <bool FLAT, int KIND>
static __global__ void __launch_bounds__(256)
k_expr_jac(const ExprProg P, ExprData ed, int n, int nblk, int ppw, int npoints, int C, const int32_t *__restrict__ dprob,
           const double *__restrict__ X, double *__restrict__ J)
{
    extern __shared__ double lds[];                               // x, the value stack, C tangent stacks
    int q, i;
    const double *xq;
    const bool on = place_staged<FLAT>(ed.m, n, nblk, ppw, npoints, X, lds, q, i, xq);
    const int qc = min(q, npoints - 1), ic = min(i, ed.m - 1);
    const int p = dprob ? dprob[qc] : qc;
    const size_t at = (size_t)p * ed.m + ic;
    double tv[NLH_EXPR_MAX_VARS];
    expr_load_vars(ed, P.nvar, at, ic, tv);
    const double w = ed.w ? ed.w[at] : 1.0;
    if (!on) return;
    const size_t m = (size_t)ed.m;
    const bool hw = ed.w != nullptr;
    double *vs = lds + (FLAT ? ppw : 1) * n + threadIdx.x;
    double *ts = vs + P.depth * 256;
    double *Jq = J + (size_t)q * m * n + i;
    const uint32_t root = P.mask[P.ninstr - 1];
    int slot = 0;                                                 // the slot the root ends in (a skipped pass reads none)
    for (int j0 = 0; j0 < n; j0 += C) {
        const int cc = min(C, n - j0);
        if ((root >> j0) & (cc >= 32 ? 0xffffffffu : (1u << cc) - 1u)) expr_run<true, KIND>(P, xq, tv, vs, ts, j0, cc, slot);
        for (int c = 0; c < cc; ++c) {
            const double d = (root >> (j0 + c)) & 1u ? ts[(c * P.depth + (KIND >= EXPR_DEFS ? slot : 0)) * 256] : 0.0;
            Jq[(size_t)(j0 + c) * m] = hw ? w * d : d;
        }
    }
}
