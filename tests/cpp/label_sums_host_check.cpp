// label_sums_host_check.cpp -- gsim_label_silhouette and gsim_label_medoids on hand-made inputs, with buffers of exactly the sizes the
// header promises.  A stand-alone program: tests/test_label_sums_host.py compiles it TOGETHER WITH
// gpusimilarity_amd/csrc/capi_label_sums_host.cpp under -fsanitize=address,undefined (that file needs the public header and fail()
// alone; fail() is defined here), so the sanitizers see the functions' own reads and writes.  No GPU, no library.
// The expected doubles are computed here by the header's operations, one at a time, through volatile temporaries.
#include "../../include/gpusim_hip.h"

#include <cmath>
#include <cstdio>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

namespace gsim_host
{
static std::string last_error;
int fail(int code, const std::string& msg)
{
    last_error = msg;
    return code;
}
} // namespace gsim_host

static int failures = 0;
#define CHECK(cond)                                                   \
    do {                                                              \
        if (!(cond)) {                                                \
            std::printf("FAILED line %d: %s\n", __LINE__, #cond);     \
            failures++;                                               \
        }                                                             \
    } while (0)

static const uint32_t NONE = GSIM_LABEL_NONE;

// exact-size heap copies: an access one element past any of them is the sanitizer's to see
template <class T> static std::unique_ptr<T[]> exact(const std::vector<T>& v)
{
    std::unique_ptr<T[]> p(new T[v.size()]);
    std::memcpy(p.get(), v.data(), v.size() * sizeof(T));
    return p;
}

static double sil_of(uint64_t own, uint32_t n_own, uint64_t oth, uint32_t n_oth)
{
    volatile double a = static_cast<double>(own) / static_cast<double>(n_own - 1u);
    a = a * 0x1p-31;
    volatile double b = static_cast<double>(oth) / static_cast<double>(n_oth);
    b = b * 0x1p-31;
    volatile double d = 1.0 - std::fmin(a, b);
    volatile double num = a - b;
    return d > 0 ? num / d : 0.0;
}

static bool same(double x, double y)
{
    return std::memcmp(&x, &y, 8) == 0;
}

int main()
{
    const uint64_t one = 1ull << 31; // q(1.0)
    // label 0: rows 0, 2, 5 (size 3); label 1: row 1 (a singleton); label 2: empty; label 3: rows 3, 6 (size 2); row 4: NONE
    const std::vector<uint32_t> labels = {0, 1, 0, 3, NONE, 0, 3};
    const std::vector<uint32_t> sizes = {3, 1, 0, 2};
    const std::vector<uint64_t> own = {one, 0, (1ull << 62) + 12345, one, 0, one + one, one};
    const std::vector<uint32_t> other = {3, 0, 1, 0, NONE, 3, NONE};
    const std::vector<uint64_t> other_q = {one, 7, 3, one + one + one, 0, one / 2, 0};
    const uint64_t n = labels.size();
    const uint32_t nlabels = 4;
    {
        auto l = exact(labels);
        auto z = exact(sizes);
        auto o = exact(own);
        auto ol = exact(other);
        auto oq = exact(other_q);
        std::unique_ptr<double[]> sil(new double[n]), lmean(new double[nlabels]);
        double mean = -1.0;
        CHECK(gsim_label_silhouette(l.get(), o.get(), ol.get(), oq.get(), z.get(), n, nlabels, sil.get(), lmean.get(), &mean) == GSIM_OK);
        const double want[7] = {sil_of(own[0], 3, other_q[0], 2), 0.0 /* a singleton */, sil_of(own[2], 3, other_q[2], 1),
                                sil_of(own[3], 2, other_q[3], 3), 0.0 /* NONE */, sil_of(own[5], 3, other_q[5], 2), 0.0 /* no other cluster */};
        for (int i = 0; i < 7; i++) CHECK(same(sil[i], want[i]));
        CHECK(same(want[0], 0.0));  // a == b == 0.5: 0 / 0.5
        CHECK(same(want[3], 0.0));  // a == b == 1.0: d == 0
        CHECK(want[2] > 0x1p29);    // own_q above 2^53 (no table gives it: a is about 2^30): the conversion rounds to nearest even
        volatile double s0 = 0.0;
        s0 = s0 + want[0];
        s0 = s0 + want[2];
        s0 = s0 + want[5];
        CHECK(same(lmean[0], s0 / 3.0) && same(lmean[1], 0.0) && same(lmean[2], 0.0));
        volatile double s3 = 0.0;
        s3 = s3 + want[3];
        s3 = s3 + want[6];
        CHECK(same(lmean[3], s3 / 2.0));
        volatile double t = 0.0;
        for (int i = 0; i < 7; i++)
            if (labels[i] != NONE) t = t + want[i];
        CHECK(same(mean, t / 6.0));
        // label_mean and mean may be NULL
        CHECK(gsim_label_silhouette(l.get(), o.get(), ol.get(), oq.get(), z.get(), n, nlabels, sil.get(), nullptr, nullptr) == GSIM_OK);
        // refused, nothing written
        std::unique_ptr<double[]> sil2(new double[n]);
        for (uint64_t i = 0; i < n; i++) sil2[i] = 77.0;
        std::vector<uint32_t> bad = other;
        bad[0] = 0; // the row's own label
        auto b1 = exact(bad);
        CHECK(gsim_label_silhouette(l.get(), o.get(), b1.get(), oq.get(), z.get(), n, nlabels, sil2.get(), nullptr, nullptr) == GSIM_ERR_INVALID);
        bad[0] = 4; // not below nlabels
        auto b2 = exact(bad);
        CHECK(gsim_label_silhouette(l.get(), o.get(), b2.get(), oq.get(), z.get(), n, nlabels, sil2.get(), nullptr, nullptr) == GSIM_ERR_INVALID);
        bad[0] = 2; // without rows
        auto b3 = exact(bad);
        CHECK(gsim_label_silhouette(l.get(), o.get(), b3.get(), oq.get(), z.get(), n, nlabels, sil2.get(), nullptr, nullptr) == GSIM_ERR_INVALID);
        std::vector<uint32_t> zbad = sizes;
        zbad[3] = 3;
        auto z2 = exact(zbad);
        CHECK(gsim_label_silhouette(l.get(), o.get(), ol.get(), oq.get(), z2.get(), n, nlabels, sil2.get(), nullptr, nullptr) == GSIM_ERR_INVALID);
        CHECK(gsim_host::last_error.find("sizes[3]") != std::string::npos);
        std::vector<uint32_t> lbad = labels;
        lbad[6] = 4;
        auto l2 = exact(lbad);
        CHECK(gsim_label_silhouette(l2.get(), o.get(), ol.get(), oq.get(), z.get(), n, nlabels, sil2.get(), nullptr, nullptr) == GSIM_ERR_INVALID);
        CHECK(gsim_label_silhouette(nullptr, o.get(), ol.get(), oq.get(), z.get(), n, nlabels, sil2.get(), nullptr, nullptr) == GSIM_ERR_INVALID);
        CHECK(gsim_label_silhouette(l.get(), o.get(), ol.get(), oq.get(), nullptr, n, nlabels, sil2.get(), nullptr, nullptr) == GSIM_ERR_INVALID);
        CHECK(gsim_label_silhouette(l.get(), o.get(), ol.get(), oq.get(), z.get(), n, 0, sil2.get(), nullptr, nullptr) == GSIM_ERR_INVALID);
        for (uint64_t i = 0; i < n; i++) CHECK(sil2[i] == 77.0);
        // no rows at all: zeros
        const std::vector<uint32_t> zero = {0, 0, 0, 0};
        auto z0 = exact(zero);
        double m0 = -1.0;
        std::unique_ptr<double[]> lm0(new double[nlabels]);
        CHECK(gsim_label_silhouette(nullptr, nullptr, nullptr, nullptr, z0.get(), 0, nlabels, nullptr, lm0.get(), &m0) == GSIM_OK);
        CHECK(m0 == 0.0 && lm0[0] == 0.0 && lm0[3] == 0.0);

        // medoids: label 0 holds the sums {2^31, 2^62 + 12345, 2^32}: row 2; label 3: rows 3 and 6 tie, the lower row wins
        std::unique_ptr<uint32_t[]> med(new uint32_t[nlabels]);
        CHECK(gsim_label_medoids(l.get(), o.get(), n, nlabels, med.get()) == GSIM_OK);
        CHECK(med[0] == 2 && med[1] == 1 && med[2] == NONE && med[3] == 3);
        med[0] = med[1] = med[2] = med[3] = 55;
        CHECK(gsim_label_medoids(l2.get(), o.get(), n, nlabels, med.get()) == GSIM_ERR_INVALID);
        CHECK(gsim_label_medoids(l.get(), nullptr, n, nlabels, med.get()) == GSIM_ERR_INVALID);
        CHECK(gsim_label_medoids(l.get(), o.get(), n, nlabels, nullptr) == GSIM_ERR_INVALID);
        CHECK(gsim_label_medoids(l.get(), o.get(), n, 0, med.get()) == GSIM_ERR_INVALID);
        CHECK(med[0] == 55 && med[3] == 55);
        CHECK(gsim_label_medoids(nullptr, nullptr, 0, nlabels, med.get()) == GSIM_OK && med[0] == NONE && med[3] == NONE);
    }
    {
        // one label only: no row has another cluster; all sums zero: the lowest row is the medoid
        const std::vector<uint32_t> lab(5, 0u), oth(5, NONE), z = {5};
        const std::vector<uint64_t> q(5, 0ull);
        auto l = exact(lab);
        auto ol = exact(oth);
        auto zz = exact(z);
        auto qq = exact(q);
        std::unique_ptr<double[]> sil(new double[5]), lm(new double[1]);
        double mean = -1.0;
        CHECK(gsim_label_silhouette(l.get(), qq.get(), ol.get(), qq.get(), zz.get(), 5, 1, sil.get(), lm.get(), &mean) == GSIM_OK);
        for (int i = 0; i < 5; i++) CHECK(sil[i] == 0.0);
        CHECK(lm[0] == 0.0 && mean == 0.0);
        std::unique_ptr<uint32_t[]> med(new uint32_t[1]);
        CHECK(gsim_label_medoids(l.get(), qq.get(), 5, 1, med.get()) == GSIM_OK && med[0] == 0);
    }
    if (failures) return 1;
    std::printf("ok\n");
    return 0;
}
