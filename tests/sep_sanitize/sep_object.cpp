// The host code of the separable object (nlh_sep_create, its refusals, _shape, _tables, _destroy) as a stand-alone program,
// to be built with the host sanitizers (see the Makefile) and run without a GPU.  Exit status 0: every check held.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../include/nonlin_hip.h"

static int failures = 0;
#define CHECK(c) do { if (!(c)) { std::printf("FAILED line %d: %s\n", __LINE__, #c); ++failures; } } while (0)

static int refused(int32_t N, std::vector<int32_t> lin)
{
    nlh_sep *sp = (nlh_sep *)0x1;
    const int rc = nlh_sep_create(N, (int32_t)lin.size(), lin.data(), &sp);
    return rc == NLH_INVALID_INPUT_ERROR && sp == nullptr;
}

int main()
{
    CHECK(refused(3, {}));                                   // L < 1
    std::vector<int32_t> many(33);
    for (int i = 0; i < 33; ++i) many[i] = i;
    CHECK(refused(40, many));                                // L > NLH_SEP_MAX_L
    CHECK(refused(3, {0, 1, 2}));                            // n < 1
    CHECK(refused(3, {0, 3}));                               // out of range
    CHECK(refused(3, {-1, 1}));
    CHECK(refused(4, {1, 1}));                               // repeated
    CHECK(refused(4, {2, 1}));                               // not ascending
    CHECK(refused(NLH_PMAP_MAX_N + 1, {0}));
    nlh_sep *sp = nullptr;
    CHECK(nlh_sep_create(3, 1, nullptr, &sp) == NLH_INVALID_INPUT_ERROR && !sp);
    const int32_t one[1] = {0};
    CHECK(nlh_sep_create(3, 1, one, nullptr) == NLH_INVALID_INPUT_ERROR);

    const int32_t lin[3] = {0, 3, 6};
    CHECK(nlh_sep_create(7, 3, lin, &sp) == 0 && sp);
    int32_t N = -1, L = -1, n = -1;
    nlh_sep_shape(sp, &N, &L, &n);
    CHECK(N == 7 && L == 3 && n == 4);
    nlh_sep_shape(sp, nullptr, nullptr, nullptr);
    std::vector<int32_t> gl(3, -1), gn(4, -1);
    CHECK(nlh_sep_tables(sp, gl.data(), gn.data()) == 0);
    CHECK(gl == std::vector<int32_t>({0, 3, 6}) && gn == std::vector<int32_t>({1, 2, 4, 5}));
    CHECK(nlh_sep_tables(sp, nullptr, nullptr) == 0);
    CHECK(nlh_sep_tables(nullptr, gl.data(), gn.data()) == NLH_INVALID_INPUT_ERROR);
    nlh_sep_destroy(sp);

    std::vector<int32_t> all(NLH_SEP_MAX_L);                 // the largest L, one nonlinear parameter, at the very end
    for (int i = 0; i < NLH_SEP_MAX_L; ++i) all[i] = i;
    CHECK(nlh_sep_create(NLH_SEP_MAX_L + 1, NLH_SEP_MAX_L, all.data(), &sp) == 0 && sp);
    std::vector<int32_t> fl(NLH_SEP_MAX_L, -1), fn(1, -1);
    CHECK(nlh_sep_tables(sp, fl.data(), fn.data()) == 0 && fl == all && fn[0] == NLH_SEP_MAX_L);
    nlh_sep_destroy(sp);
    nlh_sep_shape(nullptr, &N, &L, &n);
    CHECK(N == 0 && L == 0 && n == 0);
    nlh_sep_destroy(nullptr);
    nlh_sep_unwrap(nullptr);
    nlh_sep_ctx *ctx = (nlh_sep_ctx *)0x1;                   // what a wrap refuses before it needs a device
    CHECK(nlh_sep_wrap(nullptr, nullptr, nullptr, nullptr, nullptr, &ctx) == NLH_ERR_BAD_HANDLE && !ctx);
    std::printf(failures ? "%d checks failed\n" : "sep_object: all checks held\n", failures);
    return failures ? 1 : 0;
}
