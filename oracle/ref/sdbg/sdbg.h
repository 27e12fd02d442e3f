/*
 * sdbg/sdbg.h — TEST INFRASTRUCTURE ONLY. A stand-in for MEGAHIT's header of that name, written
 * for this project: the reference's cycle_finder.cpp is compiled against it by `make -C oracle ref`
 * (oracle/ref/ref_cf_main.cpp). It declares the nine SDBG methods CycleFinder calls and gives
 * them the conventions of DESIGN.md §2. It shares no code with oracle.cpp's Graph, on purpose:
 * the neighbour lists are made once, from the decoded symbols of every edge, and then filtered
 * by the valid bytes at query time.
 *
 * An edge is a (k+1)-mer s[0..k]; its BOSS key is ((sum s[i] << 2i, i < k) << 2) | s[k]; the
 * edge id is the position of the key in the sorted key array.
 */
#ifndef MCAAT_REF_STANDIN_SDBG_H
#define MCAAT_REF_STANDIN_SDBG_H

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <stdexcept>
#include <unordered_map>
#include <vector>

class SDBG {
  public:
    SDBG() = default;
    SDBG(int k, std::vector<uint64_t> keys, std::vector<uint16_t> mult, std::vector<uint8_t> valid)
        : k_(k), keys_(std::move(keys)), mult_(std::move(mult)), valid_(std::move(valid)) {
        if (mult_.size() != keys_.size() || valid_.size() != keys_.size())
            throw std::runtime_error("SDBG stand-in: array sizes differ");
        for (size_t i = 1; i < keys_.size(); ++i)
            if (keys_[i - 1] >= keys_[i]) throw std::runtime_error("SDBG stand-in: keys not sorted and unique");
        link();
    }

    uint64_t size() const { return keys_.size(); }
    int k() const { return k_; }
    int EdgeMultiplicity(uint64_t e) const { return mult_[e]; }
    bool IsValidEdge(uint64_t e) const { return valid_[e] != 0; }
    void SetInvalidEdge(uint64_t e) { valid_[e] = 0; }
    const std::vector<uint8_t> &valid_bytes() const { return valid_; }

    /* valid edges leaving the node this edge points to, largest id first */
    int OutgoingEdges(uint64_t e, uint64_t *out) const {
        int n = 0;
        for (int i = succ_n_[e] - 1; i >= 0; --i) {
            const uint64_t x = succ_[4 * e + i];
            if (valid_[x]) out[n++] = x;
        }
        return n;
    }
    /* valid edges entering the node this edge leaves, smallest id first */
    int IncomingEdges(uint64_t e, uint64_t *in) const {
        int n = 0;
        for (int i = 0; i < pred_n_[e]; ++i) {
            const uint64_t x = pred_[4 * e + i];
            if (valid_[x]) in[n++] = x;
        }
        return n;
    }
    int EdgeOutdegree(uint64_t e) const { uint64_t t[4]; return OutgoingEdges(e, t); }
    int EdgeIndegree(uint64_t e) const { uint64_t t[4]; return IncomingEdges(e, t); }
    bool EdgeOutdegreeZero(uint64_t e) const { return EdgeOutdegree(e) == 0; }

  private:
    /* the k+1 symbols of edge e */
    std::vector<int> symbols(uint64_t e) const {
        std::vector<int> s(k_ + 1);
        const uint64_t key = keys_[e];
        s[k_] = int(key & 3);
        for (int i = 0; i < k_; ++i) s[i] = int((key >> (2 + 2 * i)) & 3);
        return s;
    }
    /* a node's k symbols as one number, first symbol lowest */
    static uint64_t node_number(const int *s, int k) {
        uint64_t v = 0;
        for (int i = k - 1; i >= 0; --i) v = (v << 2) | uint64_t(s[i]);
        return v;
    }
    void link() {
        const uint64_t n = keys_.size();
        /* edges grouped by the node they leave; ids are pushed in ascending order */
        std::unordered_map<uint64_t, std::vector<uint64_t>> leaving;
        leaving.reserve(n);
        std::vector<uint64_t> from(n), to(n);
        for (uint64_t e = 0; e < n; ++e) {
            const std::vector<int> s = symbols(e);
            from[e] = node_number(s.data(), k_);
            to[e] = node_number(s.data() + 1, k_);
            leaving[from[e]].push_back(e);
        }
        succ_.assign(4 * n, 0); pred_.assign(4 * n, 0);
        succ_n_.assign(n, 0); pred_n_.assign(n, 0);
        /* a -> b whenever b leaves the node a points to; a ascending, so pred lists ascend too */
        for (uint64_t a = 0; a < n; ++a) {
            auto it = leaving.find(to[a]);
            if (it == leaving.end()) continue;
            for (uint64_t b : it->second) {
                if (succ_n_[a] >= 4 || pred_n_[b] >= 4) throw std::runtime_error("SDBG stand-in: degree above 4");
                succ_[4 * a + succ_n_[a]++] = b;
                pred_[4 * b + pred_n_[b]++] = a;
            }
        }
    }

    int k_ = 0;
    std::vector<uint64_t> keys_;
    std::vector<uint16_t> mult_;
    std::vector<uint8_t> valid_;
    std::vector<uint64_t> succ_, pred_; /* four slots per edge, ascending ids */
    std::vector<uint8_t> succ_n_, pred_n_;
};

#endif
