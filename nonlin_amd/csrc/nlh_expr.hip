// nlh_expr.hip -- formula models (include/nonlin_hip.h: nlh_expr_*): a model the user writes as an expression string.
// First the compiler, pure host code that needs no GPU: a recursive-descent parser of the header's grammar that emits the
// postfix of the parse tree as it goes -- no folding, no reassociation, no sharing the user did not write (a definition,
// name = expr;, is computed once and read by LOAD) -- with, per instruction, the mask of
// the parameters its subtree names and the instruction that produced its left operand (VOIGT, WHERE: its two lower operands).  Then
// the Faddeeva function's entry points (nlh_kernels_specfun.h; J0 .. LOG1P: nlh_kernels_specfun2.h), the launchers of the open
// device-residual path (kernels and arithmetic: nlh_kernels_expr.h), which form a call runs and how many Jacobian
// columns a pass carries, model values (nlh_expr_eval_batch) and the eight one-call fits nlh_expr_fit_batch*: a formula as
// the FitSource of the pipeline (nlh_fit.hip).  The model object that owns its program and data is nlh_expr_model_create
// (nlh_model.hip).
#include "nlh_internal.h"
#include "nlh_launch.h"
#include "nlh_kernels_expr.h"

#include <locale.h>

// ---------------------------------------------------------------------------------------------------------------------
// the compiler
// ---------------------------------------------------------------------------------------------------------------------
static thread_local std::string expr_err;
const char *nlh_expr_error(void) { return expr_err.c_str(); }

static const struct { const char *name; int arity; } EXPR_FUNCS[] = {
    {"exp", 1}, {"log", 1}, {"sqrt", 1}, {"sin", 1}, {"cos", 1}, {"tanh", 1}, {"atan", 1}, {"abs", 1},   // NLH_EXPR_EXP ..
    {"erf", 1}, {"erfc", 1}, {"erfcx", 1}, {"voigt", 3},                                                 // NLH_EXPR_ERF ..
    {"pow", 2}, {"atan2", 2}, {"min", 2}, {"max", 2}, {"where", 3},                                      // NLH_EXPR_POW ..
    {"j0", 1}, {"j1", 1}, {"i0e", 1}, {"i1e", 1}, {"lgamma", 1}, {"expm1", 1}, {"log1p", 1}};            // NLH_EXPR_J0 .. (LOAD lies between)
static const int EXPR_FUNCS_OLD = NLH_EXPR_WHERE - NLH_EXPR_EXP + 1;   // the functions numbered on from NLH_EXPR_EXP

namespace {
struct ExprFail {};

struct ExprParser {
    const char *s;
    size_t at = 0;
    std::vector<std::string> vars, params, defs;   // defs[k]: the name of statement k, whose value stays in slot k
    ExprProg *P;
    int nconst = 0, sp = 0;
    int root[NLH_EXPR_MAX_DEPTH + 1];          // the instruction that produced each stack slot

    [[noreturn]] void fail(size_t col, const std::string &msg)
    {
        expr_err = "col " + std::to_string(col) + ": " + msg;
        throw ExprFail();
    }
    void blanks() { while (s[at] == ' ' || s[at] == '\t' || s[at] == '\n' || s[at] == '\r') ++at; }
    char peek() { blanks(); return s[at]; }

    void emit(size_t col, int op, int arg, int pops)
    {
        if (P->ninstr >= NLH_EXPR_MAX_INSTR) fail(col, "more than " + std::to_string(NLH_EXPR_MAX_INSTR) + " instructions");
        const int pc = P->ninstr++;
        uint32_t mask = op == NLH_EXPR_PARAM ? 1u << arg : 0u;
        int aroot = 0, broot = 0;
        if (op == NLH_EXPR_LOAD) { aroot = root[arg]; mask = P->mask[aroot]; }   // a leaf that names its definition's producer
        else if (pops == 3) {                       // VOIGT: x, sigma, gamma; WHERE: c, a, b
            aroot = root[sp - 3]; broot = root[sp - 2];
            mask = P->mask[aroot] | P->mask[broot] | P->mask[root[sp - 1]];
        }
        else if (pops == 2) { aroot = root[sp - 2]; mask = P->mask[aroot] | P->mask[root[sp - 1]]; }
        else if (pops == 1) mask = P->mask[root[sp - 1]];
        sp -= pops;
        if (sp >= NLH_EXPR_MAX_DEPTH) fail(col, "the evaluation stack gets deeper than " + std::to_string(NLH_EXPR_MAX_DEPTH));
        root[sp++] = pc;
        if (sp > P->depth) P->depth = sp;
        P->code[pc] = (uint32_t)op | ((uint32_t)(arg & 0xff) << 8) | ((uint32_t)aroot << 16) | ((uint32_t)broot << 24);
        P->mask[pc] = mask;
    }
    int constant(size_t col, double v)
    {
        if (nconst >= NLH_EXPR_MAX_CONST) fail(col, "more than " + std::to_string(NLH_EXPR_MAX_CONST) + " constants");
        P->consts[nconst] = v;
        return nconst++;
    }
    static bool digit(char c) { return c >= '0' && c <= '9'; }
    static bool alpha(char c) { return (c >= 'a' && c <= 'z') || (c >= 'A' && c <= 'Z') || c == '_'; }
    double number(size_t *col)
    {
        blanks();
        *col = at;
        if (!(digit(s[at]) || (s[at] == '.' && digit(s[at + 1])))) fail(at, s[at] ? std::string("a number expected at '") + s[at] + "'" : "a number expected at the end");
        static const locale_t c_locale = newlocale(LC_ALL_MASK, "C", (locale_t)0);
        char *end = nullptr;
        const double v = strtod_l(s + at, &end, c_locale);
        if (end == s + at) fail(at, "a number expected");
        at = (size_t)(end - s);
        return v;
    }

    // formula := { name '=' expr ';' } expr.  Statement k is compiled with k slots in use, so its root lands in slot k and
    // stays there: a definition needs no store, the next statement evaluates on top of it, the model value ends in slot ndef.
    void formula()
    {
        for (;;) {
            blanks();
            size_t e = at;
            if (alpha(s[e])) while (alpha(s[e]) || digit(s[e])) ++e;
            size_t q = e;
            while (s[q] == ' ' || s[q] == '\t' || s[q] == '\n' || s[q] == '\r') ++q;
            if (e == at || s[q] != '=') break;                  // the last statement: the model value
            const size_t col = at;
            const std::string name(s + at, e - at);
            for (const auto &f : EXPR_FUNCS)
                if (name == f.name) fail(col, "'" + name + "' is a function");
            if (name == "pi") fail(col, "'pi' is the constant");
            for (const auto &v : vars)
                if (name == v) fail(col, "'" + name + "' is a variable");
            for (const auto &p : params)
                if (name == p) fail(col, "'" + name + "' is a parameter");
            for (const auto &d : defs)
                if (name == d) fail(col, "'" + name + "' is already defined");
            at = q + 1;
            expr();
            if (peek() != ';') fail(at, "';' expected after the definition of '" + name + "'");
            ++at;
            defs.push_back(name);                               // (usable from the next statement on)
        }
        expr();
        if (peek()) fail(at, std::string("unexpected '") + s[at] + "'");
    }
    void expr()
    {
        term();
        for (char c = peek(); c == '+' || c == '-'; c = peek()) {
            const size_t col = at++;
            term();
            emit(col, c == '+' ? NLH_EXPR_ADD : NLH_EXPR_SUB, 0, 2);
        }
    }
    void term()
    {
        unary();
        for (char c = peek(); c == '*' || c == '/'; c = peek()) {
            const size_t col = at++;
            unary();
            emit(col, c == '*' ? NLH_EXPR_MUL : NLH_EXPR_DIV, 0, 2);
        }
    }
    void unary()
    {
        const char c = peek();
        if (c == '-' || c == '+') {
            const size_t col = at++;
            unary();
            if (c == '-') emit(col, NLH_EXPR_NEG, 0, 1);
            return;
        }
        power();
    }
    void power()
    {
        atom();
        if (peek() != '^') return;
        const size_t col = at++;
        bool neg = false;
        if (peek() == '-') { neg = true; ++at; }
        size_t ncol;
        const char x = peek();                 // '^' takes a literal: a name or '(' here is the exponent pow(a, b) takes
        if (alpha(x) || x == '(') fail(at, std::string("a number expected at '") + x + "': '^' takes a literal exponent, write pow(a, b)");
        const double v = number(&ncol);
        if (v >= 2.0 && v <= 16.0 && v == (double)(int)v) emit(col, NLH_EXPR_IPOW, neg ? -(int)v : (int)v, 1);
        else emit(col, NLH_EXPR_POWC, constant(ncol, neg ? -v : v), 1);
        if (peek() == '^') fail(at, "a power of a power needs parentheses");
    }
    void atom()
    {
        const char c = peek();
        const size_t col = at;
        if (c == '(') {
            ++at;
            expr();
            if (peek() != ')') fail(at, "')' expected");
            ++at;
            return;
        }
        if (digit(c) || c == '.') {
            size_t ncol;
            const double v = number(&ncol);
            emit(col, NLH_EXPR_CONST, constant(col, v), 0);
            return;
        }
        if (!alpha(c)) fail(at, c ? std::string("unexpected '") + c + "'" : "unexpected end of the formula");
        size_t e = at;
        while (alpha(s[e]) || digit(s[e])) ++e;
        const std::string name(s + at, e - at);
        at = e;
        for (size_t f = 0; f < sizeof(EXPR_FUNCS) / sizeof(EXPR_FUNCS[0]); ++f)
            if (name == EXPR_FUNCS[f].name) {
                if (peek() != '(') fail(at, "'(' expected after the function '" + name + "'");
                ++at;
                const int op = (int)f < EXPR_FUNCS_OLD ? NLH_EXPR_EXP + (int)f : NLH_EXPR_J0 + ((int)f - EXPR_FUNCS_OLD), want = EXPR_FUNCS[f].arity;
                const std::string takes = "'" + name + "' takes " + (want == 1 ? "one argument" : (want == 2 ? "two arguments" : "three arguments"));
                int have = 1;
                expr();
                for (; peek() == ','; ++have) {
                    if (have == want) fail(at, takes);
                    ++at;
                    expr();
                }
                if (peek() != ')') fail(at, "')' expected");
                if (have != want) fail(at, takes);
                ++at;
                emit(col, op, 0, want);
                return;
            }
        if (name == "pi") { emit(col, NLH_EXPR_CONST, constant(col, 3.14159265358979323846), 0); return; }
        for (size_t v = 0; v < vars.size(); ++v)
            if (name == vars[v]) { emit(col, NLH_EXPR_VAR, (int)v, 0); return; }
        for (size_t k = 0; k < params.size(); ++k)
            if (name == params[k]) { emit(col, NLH_EXPR_PARAM, (int)k, 0); return; }
        for (size_t k = 0; k < defs.size(); ++k)
            if (name == defs[k]) { emit(col, NLH_EXPR_LOAD, (int)k, 0); return; }
        fail(col, "unknown name '" + name + "'");
    }
};

// a comma-separated list of names; false with the message set
bool expr_names(const char *what, const char *list, size_t most, const std::vector<std::string> &others, std::vector<std::string> &out)
{
    auto fail = [&](size_t col, const std::string &msg) {
        expr_err = std::string(what) + " col " + std::to_string(col) + ": " + msg;
        return false;
    };
    if (!list) return fail(0, "no list");
    size_t at = 0;
    for (;;) {
        while (list[at] == ' ' || list[at] == '\t') ++at;
        const size_t col = at;
        if (!ExprParser::alpha(list[at])) return fail(col, list[at] && list[at] != ',' ? std::string("unexpected '") + list[at] + "'" : "a name expected");
        while (ExprParser::alpha(list[at]) || ExprParser::digit(list[at])) ++at;
        const std::string name(list + col, at - col);
        if (name == "pi") return fail(col, "'pi' is the constant");
        for (const auto &f : EXPR_FUNCS)
            if (name == f.name) return fail(col, "'" + name + "' is a function");
        for (const auto &o : out)
            if (name == o) return fail(col, "duplicate name '" + name + "'");
        for (const auto &o : others)
            if (name == o) return fail(col, "'" + name + "' is in both lists");
        if (out.size() >= most) return fail(col, "more than " + std::to_string(most) + " names");
        out.push_back(name);
        while (list[at] == ' ' || list[at] == '\t') ++at;
        if (!list[at]) return true;
        if (list[at] != ',') return fail(at, std::string("unexpected '") + list[at] + "'");
        ++at;
    }
}
}   // namespace

int nlh_expr_compile(const char *formula, const char *vars, const char *params, nlh_expr **e)
{
    if (e) *e = nullptr;
    expr_err.clear();
    if (!e || !formula) { expr_err = "col 0: no formula"; return NLH_INVALID_INPUT_ERROR; }
    nlh_expr *x = new nlh_expr();
    memset(x, 0, sizeof(*x));
    ExprParser ps;
    ps.s = formula; ps.P = &x->prog;
    if (!expr_names("vars", vars, NLH_EXPR_MAX_VARS, {}, ps.vars) || !expr_names("params", params, NLH_EXPR_MAX_PARAMS, ps.vars, ps.params)) {
        delete x;
        return NLH_INVALID_INPUT_ERROR;
    }
    try {
        ps.formula();
    } catch (const ExprFail &) {
        delete x;
        return NLH_INVALID_INPUT_ERROR;
    }
    x->prog.nvar = (int32_t)ps.vars.size();
    x->prog.nparams = (int32_t)ps.params.size();
    x->nconst = ps.nconst;
    x->ndef = (int32_t)ps.defs.size();
    for (int i = 0; i < x->prog.ninstr; ++i)
        if (EXPR_OP(x->prog.code[i]) >= NLH_EXPR_J0) x->sf2 = 1;
    *e = x;
    return 0;
}

void nlh_expr_destroy(nlh_expr *e) { delete e; }

void nlh_expr_shape(const nlh_expr *e, int32_t *nvar, int32_t *nparams, int32_t *ninstr, int32_t *nconst, int32_t *depth)
{
    if (nvar) *nvar = e ? e->prog.nvar : 0;
    if (nparams) *nparams = e ? e->prog.nparams : 0;
    if (ninstr) *ninstr = e ? e->prog.ninstr : 0;
    if (nconst) *nconst = e ? e->nconst : 0;
    if (depth) *depth = e ? e->prog.depth : 0;
}

int nlh_expr_program(const nlh_expr *e, int32_t *op, int32_t *arg, double *consts)
{
    if (!e) return NLH_INVALID_INPUT_ERROR;
    for (int i = 0; i < e->prog.ninstr; ++i) {
        if (op) op[i] = EXPR_OP(e->prog.code[i]);
        if (arg) arg[i] = EXPR_ARG(e->prog.code[i]);
    }
    if (consts) memcpy(consts, e->prog.consts, sizeof(double) * e->nconst);
    return 0;
}

int nlh_expr_roots(const nlh_expr *e, int32_t *aroot, int32_t *broot)
{
    if (!e) return NLH_INVALID_INPUT_ERROR;
    for (int i = 0; i < e->prog.ninstr; ++i) {
        if (aroot) aroot[i] = EXPR_AROOT(e->prog.code[i]);
        if (broot) broot[i] = EXPR_BROOT(e->prog.code[i]);
    }
    return 0;
}

int nlh_expr_masks(const nlh_expr *e, uint32_t *mask)
{
    if (!e || !mask) return NLH_INVALID_INPUT_ERROR;
    memcpy(mask, e->prog.mask, sizeof(uint32_t) * e->prog.ninstr);
    return 0;
}

// ---------------------------------------------------------------------------------------------------------------------
// the Faddeeva function (nlh_kernels_specfun.h): the host entry, the table, a thread per element on the device
// ---------------------------------------------------------------------------------------------------------------------
int nlh_faddeeva(double re, double im, double *wre, double *wim)
{
    if (!wre || !wim || !(im >= 0.0)) return NLH_INVALID_INPUT_ERROR;
    faddeeva_w(re, im, wre, wim);
    return 0;
}

void nlh_faddeeva_table(double *L, double *a40)
{
    if (L) *L = NLH_FADDEEVA_L;
    if (a40) memcpy(a40, NLH_FADDEEVA_A, sizeof(NLH_FADDEEVA_A));
}

int nlh_faddeeva_batch(nlh_handle *h, int64_t count, const double *dre, const double *dim, double *dwre, double *dwim)
{
    if (!h) return NLH_ERR_BAD_HANDLE;
    if (count < 0) return NLH_INVALID_INPUT_ERROR;
    if (count == 0) return 0;
    if (!dre || !dim || !dwre || !dwim) return NLH_INVALID_INPUT_ERROR;
    if ((count + 255) / 256 > 0x7fffffffLL) return NLH_ARRAY_SIZE_ERROR;
    HIPCHK(h, hipSetDevice(h->device));
    hipLaunchKernelGGL(k_faddeeva, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, h->stream, (long long)count, dre, dim, dwre, dwim);
    HIPCHK(h, hipGetLastError());
    return 0;
}

// ---------------------------------------------------------------------------------------------------------------------
// the launchers
// ---------------------------------------------------------------------------------------------------------------------
void nlh_expr_init_device(int lds_max)
{
    for (const void *k : {(const void *)k_expr_fcn<false, EXPR_PLAIN>, (const void *)k_expr_fcn<true, EXPR_PLAIN>, (const void *)k_expr_fcn<false, EXPR_DEFS>,
                          (const void *)k_expr_fcn<true, EXPR_DEFS>, (const void *)k_expr_fcn<false, EXPR_SF2>, (const void *)k_expr_fcn<true, EXPR_SF2>,
                          (const void *)k_expr_jac<false, EXPR_PLAIN>, (const void *)k_expr_jac<true, EXPR_PLAIN>, (const void *)k_expr_jac<false, EXPR_DEFS>,
                          (const void *)k_expr_jac<true, EXPR_DEFS>, (const void *)k_expr_jac<false, EXPR_SF2>, (const void *)k_expr_jac<true, EXPR_SF2>})
        (void)hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, lds_max);
}

// The form a launch runs, as the curve models choose it: flat (several points per workgroup) while two points or more fit
// a workgroup's 256 threads.  NLH_EXPR_FORM = row | flat (environment, read at every call; tests) forces a form for the
// sizes it can hold (flat: m <= 256).
static bool expr_flat(int m) { return launch_flat("NLH_EXPR_FORM", m); }

// Columns of the Jacobian a pass over the program carries.  A stack is depth * 256 doubles; a pass needs 1 + C of them
// besides the x of the workgroup's points.  The most columns, 8 and n at most, with which that stays within half of
// NLH_LDS_MAX, so that two workgroups share a compute unit; one column under the whole of it where even that does not fit
// half (depth 16: 65,536 bytes of stacks).  NLH_EXPR_CHUNK (environment; tests) asks for fewer.
static int expr_chunk(int depth, int n, size_t xbytes)
{
    const size_t stack = sizeof(double) * 256 * (size_t)depth, half = (size_t)NLH_LDS_MAX / 2;
    int C = half > xbytes + stack ? (int)((half - xbytes) / stack) - 1 : 0;
    C = std::max(1, std::min(C, std::min(n, 8)));
    if (const char *e = getenv("NLH_EXPR_CHUNK")) {
        const int want = atoi(e);
        if (want >= 1 && want < C) C = want;
    }
    return C;
}

// The launch shape of a call: the form, the points a flat workgroup holds, the row blocks of a point, the grid's x, the
// columns a Jacobian pass carries (0: the residual kernel) and the dynamic LDS -- x of the workgroup's points, the value
// stack, C tangent stacks.  Pure host code: expr_launch dispatches through it, nlh_expr_plan reports it.
struct ExprPlan {
    bool flat;
    int ppw, nblk, C;
    size_t grid, lds;
};
static int expr_plan(int depth, int n, int m, int npoints, bool jac, ExprPlan &p)
{
    if (depth < 1 || depth > NLH_EXPR_MAX_DEPTH || n < 1 || n > NLH_EXPR_MAX_PARAMS || m < 1 || npoints < 0) return NLH_INVALID_INPUT_ERROR;
    if ((size_t)npoints * ((size_t)(m + 255) / 256) > 0x7fffffffu) return NLH_ARRAY_SIZE_ERROR;
    p.flat = expr_flat(m);
    p.ppw = p.flat ? 256 / m : 1; p.nblk = p.flat ? 1 : (m + 255) / 256;
    p.grid = p.flat ? (size_t)((npoints + p.ppw - 1) / p.ppw) : (size_t)npoints * p.nblk;
    const size_t xbytes = sizeof(double) * (size_t)p.ppw * n, stack = sizeof(double) * 256 * (size_t)depth;
    p.C = jac ? expr_chunk(depth, n, xbytes) : 0;
    p.lds = xbytes + stack * (size_t)(1 + p.C);
    return 0;
}

int32_t nlh_expr_plan(int32_t depth, int32_t n, int32_t m, int32_t npoints, int32_t jac, int32_t *flat, int32_t *ppw, int32_t *nblk,
                      int64_t *grid, int32_t *chunk, int64_t *lds_bytes)
{
    if (!flat || !ppw || !nblk || !grid || !chunk || !lds_bytes) return NLH_INVALID_INPUT_ERROR;
    ExprPlan p;
    if (const int rc = expr_plan(depth, n, m, npoints, jac != 0, p)) return rc;
    *flat = p.flat; *ppw = p.ppw; *nblk = p.nblk; *grid = (int64_t)p.grid; *chunk = p.C; *lds_bytes = (int64_t)p.lds;
    return 0;
}

// Checks everything, launches nothing when anything is wrong.  y == nullptr: model values (no data term, no weights).
static int expr_launch(bool jac, const nlh_expr *e, int shared_t, int m, int64_t stride, const double *t, const double *y, const double *w,
                       int32_t npoints, const int32_t *dprob, int32_t n, const double *dX, double *out, hipStream_t s)
{
    if (!e || e->prog.nparams != n || m < 1 || !t || !dX || !out) return NLH_INVALID_INPUT_ERROR;
    if (stride == 0 && shared_t) stride = m;
    if (e->prog.nvar > 1 && stride < m) return NLH_INVALID_INPUT_ERROR;
    if (npoints <= 0) return 0;
    ExprPlan p;
    if (const int rc = expr_plan(e->prog.depth, n, m, npoints, jac, p)) return rc;
    ExprData ed;
    ed.shared_t = shared_t != 0; ed.m = m; ed.tstride = stride; ed.t = t; ed.y = y; ed.w = w;
    const dim3 grid((unsigned)p.grid);
    const int ppw = p.ppw, nblk = p.nblk, C = p.C;
    // (a program without definitions runs the instantiations that know none, one without J0 .. LOG1P those that know none
    // of them: the kernels they always ran)
    const auto fcn = e->sf2 ? (p.flat ? k_expr_fcn<true, EXPR_SF2> : k_expr_fcn<false, EXPR_SF2>)
                   : e->ndef ? (p.flat ? k_expr_fcn<true, EXPR_DEFS> : k_expr_fcn<false, EXPR_DEFS>)
                             : (p.flat ? k_expr_fcn<true, EXPR_PLAIN> : k_expr_fcn<false, EXPR_PLAIN>);
    const auto jk = e->sf2 ? (p.flat ? k_expr_jac<true, EXPR_SF2> : k_expr_jac<false, EXPR_SF2>)
                  : e->ndef ? (p.flat ? k_expr_jac<true, EXPR_DEFS> : k_expr_jac<false, EXPR_DEFS>)
                            : (p.flat ? k_expr_jac<true, EXPR_PLAIN> : k_expr_jac<false, EXPR_PLAIN>);
    if (!jac) hipLaunchKernelGGL(fcn, grid, dim3(256), p.lds, s, e->prog, ed, n, nblk, ppw, npoints, dprob, dX, out);
    else hipLaunchKernelGGL(jk, grid, dim3(256), p.lds, s, e->prog, ed, n, nblk, ppw, npoints, C, dprob, dX, out);
    return 0;
}

int nlh_expr_device_fcn(void *ctx, void *hip_stream, int32_t npoints, const int32_t *dprob, int32_t n, const double *dX, int32_t m,
                        double *dF)
{
    const nlh_expr_ctx *c = (const nlh_expr_ctx *)ctx;
    if (!c || m != c->m || !c->dy || !dprob) return NLH_INVALID_INPUT_ERROR;
    return expr_launch(false, c->e, c->shared_t, c->m, c->dt_stride, c->dt, c->dy, c->dw, npoints, dprob, n, dX, dF, (hipStream_t)hip_stream);
}

int nlh_expr_device_jac(void *ctx, void *hip_stream, int32_t npoints, const int32_t *dprob, int32_t n, const double *dX, int32_t m,
                        double *dJ)
{
    const nlh_expr_ctx *c = (const nlh_expr_ctx *)ctx;
    if (!c || m != c->m || !c->dy || !dprob) return NLH_INVALID_INPUT_ERROR;
    return expr_launch(true, c->e, c->shared_t, c->m, c->dt_stride, c->dt, c->dy, c->dw, npoints, dprob, n, dX, dJ, (hipStream_t)hip_stream);
}

int nlh_expr_eval_batch(nlh_handle *h, const nlh_expr *e, int32_t nprob, int32_t npts, const double *dt, int32_t shared_t, const double *dx,
                        double *dy)
{
    if (!h) return NLH_ERR_BAD_HANDLE;
    if (!e || nprob < 0 || npts < 1) return NLH_INVALID_INPUT_ERROR;
    const int32_t n = e->prog.nparams;
    if (nprob == 0) return 0;
    int rc;
    if (!dt || !dx || !dy) return NLH_INVALID_INPUT_ERROR;
    HIPCHK(h, hipSetDevice(h->device));
    const int64_t stride = shared_t ? (int64_t)npts : (int64_t)nprob * npts;
    if ((rc = expr_launch(false, e, shared_t, npts, stride, dt, nullptr, nullptr, nprob, nullptr, n, dx, dy, h->stream))) return rc;
    HIPCHK(h, hipGetLastError());
    return 0;
}

// The formula itself as a launcher pair -- no data term, no weights: what nlh_expr_eval_batch launches, with a problem list
// -- for the band (nlh_band.hip), on a context of the call's own.
static int expr_value_fcn(void *ctx, void *hip_stream, int32_t npoints, const int32_t *dprob, int32_t n, const double *dX, int32_t m,
                          double *dF)
{
    const nlh_expr_ctx *c = (const nlh_expr_ctx *)ctx;
    if (!c || m != c->m || !dprob) return NLH_INVALID_INPUT_ERROR;
    return expr_launch(false, c->e, c->shared_t, c->m, c->dt_stride, c->dt, nullptr, nullptr, npoints, dprob, n, dX, dF, (hipStream_t)hip_stream);
}

static int expr_value_jac(void *ctx, void *hip_stream, int32_t npoints, const int32_t *dprob, int32_t n, const double *dX, int32_t m,
                          double *dJ)
{
    const nlh_expr_ctx *c = (const nlh_expr_ctx *)ctx;
    if (!c || m != c->m || !dprob) return NLH_INVALID_INPUT_ERROR;
    return expr_launch(true, c->e, c->shared_t, c->m, c->dt_stride, c->dt, nullptr, nullptr, npoints, dprob, n, dX, dJ, (hipStream_t)hip_stream);
}

int nlh_expr_band_batch(nlh_handle *h, const nlh_expr *e, int32_t nprob, int32_t npts, const double *dt, int32_t shared_t, const double *dx,
                        const double *dcov, const double *dnoise, double *dy, double *dsd)
{
    if (!h) return NLH_ERR_BAD_HANDLE;
    if (!e || nprob < 0 || npts < 1) return NLH_INVALID_INPUT_ERROR;
    if (nprob == 0) return 0;
    if (!dt || !dx || !dcov || !dsd) return NLH_INVALID_INPUT_ERROR;
    nlh_expr_ctx c;
    c.e = e; c.shared_t = shared_t != 0; c.m = npts; c.dt = dt; c.dy = nullptr; c.dw = nullptr;
    c.dt_stride = shared_t ? (int64_t)npts : (int64_t)nprob * npts;
    return nlh_propagate_batch_device(h, nprob, npts, e->prog.nparams, expr_value_fcn, expr_value_jac, &c, dx, dcov, dnoise, dy, dsd);
}

// ---------------------------------------------------------------------------------------------------------------------
// fit + errors: the pipeline of nlh_fit.hip on a formula
// ---------------------------------------------------------------------------------------------------------------------
static void expr_bind(void *ctx, const double *dt, const double *dy, const double *dw, int32_t p0)
{
    nlh_expr_ctx *c = (nlh_expr_ctx *)ctx;
    const size_t at = (size_t)p0 * c->m;
    c->dt = c->shared_t ? dt : dt + at;
    c->dy = dy + at;
    c->dw = dw ? dw + at : nullptr;
}

static int expr_fit(nlh_handle *h, const nlh_options *opts, const nlh_expr *e, int32_t analytic, const FitArgs &a, bool host)
{
    nlh_expr_ctx c;                                               // (its data pointers: expr_bind, before every run of problems)
    c.e = e; c.shared_t = a.shared_t != 0; c.m = a.m;
    c.dt_stride = a.shared_t ? (int64_t)a.m : (int64_t)a.nprob * a.m;   // (a run of problems keeps the whole batch's stride)
    const FitSource src = {e ? e->prog.nparams : -1, e ? (size_t)e->prog.nvar : 0, "formula fit", nlh_expr_device_fcn,
                           analytic ? nlh_expr_device_jac : nullptr, &c, expr_bind};
    return nlh_fit_run(h, opts, src, a, host);
}

int nlh_expr_fit_batch(nlh_handle *h, const nlh_options *opts, const nlh_expr *e, int32_t nprob, int32_t m, const double *dt,
                       int32_t shared_t, const double *dy, const double *dw, int32_t analytic, const double *xl, const double *xu,
                       double *dx, double *dfvec, double *dsigma, double *dcov, double *dchi2, int32_t *drank, nlh_iteration_behavior *ib,
                       int32_t *status)
{
    return expr_fit(h, opts, e, analytic, {nprob, m, dt, shared_t, dy, dw, xl, xu, nullptr, NLH_LOSS_LINEAR, nullptr, 0, dx, dfvec, dsigma, dcov,
                                           dchi2, drank, ib, status}, false);
}

int nlh_expr_fit_batch_h(nlh_handle *h, const nlh_options *opts, const nlh_expr *e, int32_t nprob, int32_t m, const double *t,
                         int32_t shared_t, const double *y, const double *w, int32_t analytic, const double *xl, const double *xu, double *x,
                         double *fvec, double *sigma, double *cov, double *chi2, int32_t *rank, nlh_iteration_behavior *ib, int32_t *status)
{
    return expr_fit(h, opts, e, analytic, {nprob, m, t, shared_t, y, w, xl, xu, nullptr, NLH_LOSS_LINEAR, nullptr, 0, x, fvec, sigma, cov, chi2,
                                           rank, ib, status}, true);
}

int nlh_expr_fit_batch_pmap(nlh_handle *h, const nlh_options *opts, const nlh_expr *e, int32_t nprob, int32_t m, const double *dt,
                            int32_t shared_t, const double *dy, const double *dw, int32_t analytic, const double *xl, const double *xu,
                            const nlh_pmap *pm, double *dx, double *dfvec, double *dsigma, double *dcov, double *dchi2, int32_t *drank,
                            nlh_iteration_behavior *ib, int32_t *status)
{
    return expr_fit(h, opts, e, analytic, {nprob, m, dt, shared_t, dy, dw, xl, xu, pm, NLH_LOSS_LINEAR, nullptr, 0, dx, dfvec, dsigma, dcov,
                                           dchi2, drank, ib, status}, false);
}

int nlh_expr_fit_batch_pmap_h(nlh_handle *h, const nlh_options *opts, const nlh_expr *e, int32_t nprob, int32_t m, const double *t,
                              int32_t shared_t, const double *y, const double *w, int32_t analytic, const double *xl, const double *xu,
                              const nlh_pmap *pm, double *x, double *fvec, double *sigma, double *cov, double *chi2, int32_t *rank,
                              nlh_iteration_behavior *ib, int32_t *status)
{
    return expr_fit(h, opts, e, analytic, {nprob, m, t, shared_t, y, w, xl, xu, pm, NLH_LOSS_LINEAR, nullptr, 0, x, fvec, sigma, cov, chi2, rank,
                                           ib, status}, true);
}

int nlh_expr_fit_batch_loss(nlh_handle *h, const nlh_options *opts, const nlh_expr *e, int32_t nprob, int32_t m, const double *dt,
                            int32_t shared_t, const double *dy, const double *dw, int32_t analytic, const double *xl, const double *xu,
                            const nlh_pmap *pm, int32_t loss, const double *dscale, int32_t shared_scale, double *dx, double *dfvec,
                            double *dsigma, double *dcov, double *dchi2, int32_t *drank, nlh_iteration_behavior *ib, int32_t *status)
{
    return expr_fit(h, opts, e, analytic, {nprob, m, dt, shared_t, dy, dw, xl, xu, pm, loss, dscale, shared_scale, dx, dfvec, dsigma, dcov, dchi2,
                                           drank, ib, status}, false);
}

int nlh_expr_fit_batch_loss_h(nlh_handle *h, const nlh_options *opts, const nlh_expr *e, int32_t nprob, int32_t m, const double *t,
                              int32_t shared_t, const double *y, const double *w, int32_t analytic, const double *xl, const double *xu,
                              const nlh_pmap *pm, int32_t loss, const double *scale, int32_t shared_scale, double *x, double *fvec,
                              double *sigma, double *cov, double *chi2, int32_t *rank, nlh_iteration_behavior *ib, int32_t *status)
{
    return expr_fit(h, opts, e, analytic, {nprob, m, t, shared_t, y, w, xl, xu, pm, loss, scale, shared_scale, x, fvec, sigma, cov, chi2, rank,
                                           ib, status}, true);
}

int nlh_expr_fit_batch_pois(nlh_handle *h, const nlh_options *opts, const nlh_expr *e, int32_t nprob, int32_t m, const double *dt,
    int32_t shared_t, const double *dy, const double *dw, int32_t analytic, const double *xl, const double *xu, const nlh_pmap *pm,
    double mu_floor, double *dx, double *dfvec, double *dsigma, double *dcov, double *dchi2, int32_t *drank,
    nlh_iteration_behavior *ib, int32_t *status)
{
    return expr_fit(h, opts, e, analytic, {nprob, m, dt, shared_t, dy, dw, xl, xu, pm, NLH_LOSS_LINEAR, nullptr, 0, dx, dfvec, dsigma,
                                             dcov, dchi2, drank, ib, status, NLH_STAT_POISSON, mu_floor}, false);
}

int nlh_expr_fit_batch_pois_h(nlh_handle *h, const nlh_options *opts, const nlh_expr *e, int32_t nprob, int32_t m, const double *t,
    int32_t shared_t, const double *y, const double *w, int32_t analytic, const double *xl, const double *xu, const nlh_pmap *pm,
    double mu_floor, double *x, double *fvec, double *sigma, double *cov, double *chi2, int32_t *rank,
    nlh_iteration_behavior *ib, int32_t *status)
{
    return expr_fit(h, opts, e, analytic, {nprob, m, t, shared_t, y, w, xl, xu, pm, NLH_LOSS_LINEAR, nullptr, 0, x, fvec, sigma,
                                             cov, chi2, rank, ib, status, NLH_STAT_POISSON, mu_floor}, true);
}

// The global fits: the loss (or the Poisson pair) wraps the formula per data set, the group wraps the result (nlh_fit.hip).
int nlh_expr_fit_batch_group(nlh_handle *h, const nlh_options *opts, const nlh_expr *e, int32_t nprob, int32_t m, const double *dt,
                             int32_t shared_t, const double *dy, const double *dw, int32_t analytic, const double *xl, const double *xu,
                             const nlh_group *g, int32_t loss, const double *dscale, int32_t shared_scale, int32_t stat, double mu_floor,
                             double *dx, double *dfvec, double *dsigma, double *dcov, double *dchi2, int32_t *drank,
                             nlh_iteration_behavior *ib, int32_t *status)
{
    if (h && !g) return NLH_INVALID_INPUT_ERROR;
    return expr_fit(h, opts, e, analytic, {nprob, m, dt, shared_t, dy, dw, xl, xu, nullptr, loss, dscale, shared_scale, dx, dfvec, dsigma, dcov,
                                           dchi2, drank, ib, status, stat, mu_floor, g}, false);
}

int nlh_expr_fit_batch_group_h(nlh_handle *h, const nlh_options *opts, const nlh_expr *e, int32_t nprob, int32_t m, const double *t,
                               int32_t shared_t, const double *y, const double *w, int32_t analytic, const double *xl, const double *xu,
                               const nlh_group *g, int32_t loss, const double *scale, int32_t shared_scale, int32_t stat, double mu_floor,
                               double *x, double *fvec, double *sigma, double *cov, double *chi2, int32_t *rank,
                               nlh_iteration_behavior *ib, int32_t *status)
{
    if (h && !g) return NLH_INVALID_INPUT_ERROR;
    return expr_fit(h, opts, e, analytic, {nprob, m, t, shared_t, y, w, xl, xu, nullptr, loss, scale, shared_scale, x, fvec, sigma, cov, chi2,
                                           rank, ib, status, stat, mu_floor, g}, true);
}

// The fits with an instrument response: the convolving pair wraps the model's launchers, then the loss or the Poisson pair, then
// the map or the group (nlh_fit.hip).
int nlh_expr_fit_batch_conv(nlh_handle *h, const nlh_options *opts, const nlh_expr *e, int32_t nprob, int32_t m, const double *dt,
                             int32_t shared_t, const double *dy, const double *dw, int32_t analytic, const double *xl, const double *xu,
                             const nlh_group *g, const nlh_pmap *pm, const nlh_conv *cv, int32_t loss, const double *dscale, int32_t shared_scale,
                             int32_t stat, double mu_floor, double *dx, double *dfvec, double *dsigma, double *dcov, double *dchi2,
                             int32_t *drank, nlh_iteration_behavior *ib, int32_t *status)
{
    static const nlh_conv none{};                                 // (a NULL cv: refused where the ladder checks the transform)
    return expr_fit(h, opts, e, analytic, {nprob, m, dt, shared_t, dy, dw, xl, xu, pm, loss, dscale, shared_scale, dx, dfvec, dsigma, dcov, dchi2, drank,
            ib, status, stat, mu_floor, g, cv ? cv : &none}, false);
}

int nlh_expr_fit_batch_conv_h(nlh_handle *h, const nlh_options *opts, const nlh_expr *e, int32_t nprob, int32_t m, const double *t,
                             int32_t shared_t, const double *y, const double *w, int32_t analytic, const double *xl, const double *xu,
                             const nlh_group *g, const nlh_pmap *pm, const nlh_conv *cv, int32_t loss, const double *scale, int32_t shared_scale,
                             int32_t stat, double mu_floor, double *x, double *fvec, double *sigma, double *cov, double *chi2,
                             int32_t *rank, nlh_iteration_behavior *ib, int32_t *status)
{
    static const nlh_conv none{};                                 // (a NULL cv: refused where the ladder checks the transform)
    return expr_fit(h, opts, e, analytic, {nprob, m, t, shared_t, y, w, xl, xu, pm, loss, scale, shared_scale, x, fvec, sigma, cov, chi2, rank,
            ib, status, stat, mu_floor, g, cv ? cv : &none}, true);
}

// The separable fits: the convolving pair, if any, wraps the model's launchers, the projecting pair wraps that (nlh_fit.hip).
int nlh_expr_fit_batch_sep(nlh_handle *h, const nlh_options *opts, const nlh_expr *e, int32_t nprob, int32_t m, const double *dt,
                           int32_t shared_t, const double *dy, const double *dw, int32_t analytic, const double *xl, const double *xu,
                           const nlh_group *g, const nlh_conv *cv, const nlh_sep *sp, double *dx, double *dfvec, double *dsigma, double *dcov,
                           double *dchi2, int32_t *drank, nlh_iteration_behavior *ib, int32_t *status)
{
    return expr_fit(h, opts, e, analytic, {nprob, m, dt, shared_t, dy, dw, xl, xu, nullptr, NLH_LOSS_LINEAR, nullptr, 0, dx, dfvec, dsigma, dcov,
                                           dchi2, drank, ib, status, NLH_STAT_LSQ, 0.0, g, cv, true, sp, nlh_expr_device_jac}, false);
}

int nlh_expr_fit_batch_sep_h(nlh_handle *h, const nlh_options *opts, const nlh_expr *e, int32_t nprob, int32_t m, const double *t,
                             int32_t shared_t, const double *y, const double *w, int32_t analytic, const double *xl, const double *xu,
                             const nlh_group *g, const nlh_conv *cv, const nlh_sep *sp, double *x, double *fvec, double *sigma, double *cov,
                             double *chi2, int32_t *rank, nlh_iteration_behavior *ib, int32_t *status)
{
    return expr_fit(h, opts, e, analytic, {nprob, m, t, shared_t, y, w, xl, xu, nullptr, NLH_LOSS_LINEAR, nullptr, 0, x, fvec, sigma, cov, chi2,
                                           rank, ib, status, NLH_STAT_LSQ, 0.0, g, cv, true, sp, nlh_expr_device_jac}, true);
}
