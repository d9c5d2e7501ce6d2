// Density clusters of stored faces in plain loops, once, for the host twin (fid_cluster_host, cluster.hip) and the stand-alone sanitizer
// driver (tests/cluster_host_driver.cpp).  Plain C++: no device header, no library call beyond <vector>.  The rule is include/faceid.h's
// (fid_gallery_cluster); tests/cluster_oracle.py is its executable form.
//
//   cosine  = the fp32 sum of the fp16 products in ASCENDING column order (a product of two fp16 values is exact in fp32, so a fused
//             multiply-add rounds like a multiply and an add).  The device sums the same products in the order of its MFMA tiles: wherever
//             the sums are exact (the +-1 / 0 probe rows of the tests) host and device are equal to the bit; elsewhere a pair whose cosine
//             lies within summation-order rounding of the threshold ((dim - 1) * 2^-24 * sum|a_i b_i|, 3e-5 for unit rows of 512) may fall
//             on either side of it.
//   borders = a non-core position goes to the cluster of the core that hits it with the HIGHEST score (lowest position among equal
//             scores): a rule, where sklearn's DBSCAN gives a border point to whichever cluster reaches it first.
#pragma once
#include <cstdint>
#include <cstring>
#include <vector>

#define FID_CLUSTER_SUMMARY_WORDS 6       // clusters, cores, borders, noise, took part, fault

inline float fid_cluster_half(uint16_t h) {
    const uint32_t sign = (uint32_t)(h & 0x8000u) << 16, exp = (h >> 10) & 31u, man = h & 0x3FFu;
    uint32_t u;
    if (exp == 0) {
        if (man == 0) {
            u = sign;
        } else {                          // subnormal: man * 2^-24, exact in fp32
            float f = (float)man * 5.9604644775390625e-08f;
            memcpy(&u, &f, 4);
            u |= sign;
        }
    } else if (exp == 31) {
        u = sign | 0x7F800000u | (man << 13);
    } else {
        u = sign | ((exp + 112u) << 23) | (man << 13);
    }
    float f;
    memcpy(&f, &u, 4);
    return f;
}

// NULL = the arguments are fine (the host twin takes any dim >= 1; the device needs dim % 32 == 0)
inline const char *fid_cluster_check(const void *rows_f16, int G, int dim, int n, float thresh, int min_pts, const int32_t *label,
                                     const int32_t *degree, const int32_t *via, const float *score, const int32_t *summary) {
    if (!rows_f16 || !label || !degree || !via || !score || !summary) return "NULL rows or output pointer";
    if (G <= 0 || dim <= 0) return "G and dim must be positive";
    if (n <= 0) return "n must be positive";
    if (min_pts < 1) return "min_pts must be >= 1";
    if (thresh != thresh) return "the threshold is NaN";
    if (!(thresh > 0.f)) return "the threshold must be > 0 (a hit needs a score > 0)";
    return nullptr;
}

// rows == NULL: positions = gallery rows 0 .. G - 1 (the caller passes n = G).  Outputs: label / degree / via int32 [n], score float [n],
// summary int32 [6].
inline void fid_cluster_table_host(const void *rows_f16, int G, int dim, const int32_t *rows, int n, float thresh, int min_pts, int32_t *label,
                                   int32_t *degree, int32_t *via, float *score, int32_t *summary) {
    const uint16_t *g = (const uint16_t *)rows_f16;
    std::vector<float> x((size_t)n * dim, 0.f);
    for (int k = 0; k < n; k++) {
        const long long row = rows ? rows[k] : k;
        unsigned any = 0;
        if (row >= 0 && row < G)
            for (int c = 0; c < dim; c++) {
                const uint16_t h = g[(size_t)row * dim + c];
                any |= h & 0x7FFFu;
                x[(size_t)k * dim + c] = fid_cluster_half(h);
            }
        degree[k] = any != 0u;
        label[k] = -1;
        via[k] = -1;
        score[k] = 0.f;
    }
    struct Hit { int32_t i, j; float s; };
    std::vector<Hit> hits;
    for (int i = 0; i < n; i++) {
        if (!degree[i]) continue;
        const float *a = &x[(size_t)i * dim];
        for (int j = i + 1; j < n; j++) {
            if (!degree[j]) continue;
            const float *b = &x[(size_t)j * dim];
            float s = 0.f;
            for (int c = 0; c < dim; c++) s += a[c] * b[c];
            if (s >= thresh && s > 0.f) hits.push_back(Hit{i, j, s});
        }
    }
    for (const Hit &h : hits) { degree[h.i]++; degree[h.j]++; }
    // union-find over the cores, the larger root under the smaller: the root of a cluster is its lowest core position
    std::vector<int32_t> parent((size_t)n);
    for (int k = 0; k < n; k++) parent[k] = k;
    auto find = [&](int32_t v) {
        while (parent[v] != v) { parent[v] = parent[parent[v]]; v = parent[v]; }
        return v;
    };
    std::vector<uint64_t> key((size_t)n, 0);      // score bits << 32 | ~position: a hit score is > 0, so its bits order like the score
    auto raise = [&](int32_t k, int32_t c, float s) {
        uint32_t u;
        memcpy(&u, &s, 4);
        const uint64_t v = ((uint64_t)u << 32) | (uint32_t)~(uint32_t)c;
        if (v > key[k]) key[k] = v;
    };
    for (const Hit &h : hits) {
        const bool ci = degree[h.i] >= min_pts, cj = degree[h.j] >= min_pts;
        if (ci && cj) {
            const int32_t a = find(h.i), b = find(h.j);
            if (a < b) parent[b] = a; else if (b < a) parent[a] = b;
        }
        if (cj) raise(h.i, h.j, h.s);
        if (ci) raise(h.j, h.i, h.s);
    }
    int32_t clusters = 0, cores = 0, borders = 0, noise = 0, part = 0;
    for (int k = 0; k < n; k++) {
        if (!degree[k]) continue;
        part++;
        if (key[k]) {
            const uint32_t u = (uint32_t)(key[k] >> 32);
            via[k] = (int32_t)~(uint32_t)key[k];
            memcpy(&score[k], &u, 4);
        }
        if (degree[k] >= min_pts) {
            cores++;
            label[k] = find(k);
            clusters += label[k] == k;
        } else if (via[k] >= 0) {
            borders++;
            label[k] = find(via[k]);
        } else {
            noise++;
        }
    }
    summary[0] = clusters; summary[1] = cores; summary[2] = borders; summary[3] = noise; summary[4] = part; summary[5] = 0;
}
