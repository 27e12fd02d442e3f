/*
 * ref_cf_main.cpp — TEST INFRASTRUCTURE ONLY. Runs the reference's own CycleFinder (its
 * src/cycle_finder.cpp, compiled in place by `make -C oracle ref`) on a graph given as arrays,
 * through the stand-in SDBG of oracle/ref/sdbg/sdbg.h, at threads = 1.
 *
 *   ref_cf run GRAPH RESULT threshold_multiplicity low_abundance cycle_max_length cycle_min_length
 *   ref_cf neighbors GRAPH RESULT
 *
 * GRAPH (little endian): "MCRG" | int32 k | uint64 n | uint64 keys[n] | uint16 mult[n] | uint8 valid[n]
 * RESULT of `run`, all uint64 unless noted:
 *   n_entries, then per entry of `results` in the map's iteration order:
 *       start, n_cycles, then per cycle: length, nodes[length]
 *   n_buckets, then per bucket of ChunkStartNodes (descending key): int64 key, count, ids[count]
 *   n, then uint8 valid[n]
 * RESULT of `neighbors`: per edge, uint64 n_out, out[n_out], n_in, in[n_in] (all edges valid or
 * not: the lists hold valid neighbours only).
 * The reference's progress lines go to stdout untouched; the line "ref_cf: second ChunkStartNodes"
 * separates the constructor's output from that of the extra ChunkStartNodes call made here.
 */
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <iostream>
#include <map>
#include <stdexcept>
#include <string>
#include <vector>

#include "cycle_finder.h"
#include "settings.h"

namespace {

void die(const std::string &msg) {
    std::fprintf(stderr, "ref_cf: %s\n", msg.c_str());
    std::exit(2);
}

void read_exact(std::FILE *f, void *p, size_t bytes) {
    if (bytes && std::fread(p, 1, bytes, f) != bytes) die("graph file is truncated");
}

SDBG read_graph(const char *path) {
    std::FILE *f = std::fopen(path, "rb");
    if (!f) die(std::string("cannot open ") + path);
    char magic[4];
    int32_t k = 0;
    uint64_t n = 0;
    read_exact(f, magic, 4);
    if (std::memcmp(magic, "MCRG", 4) != 0) die("not a graph file");
    read_exact(f, &k, 4);
    read_exact(f, &n, 8);
    if (k < 2 || k > 30) die("k out of range");
    std::vector<uint64_t> keys(n);
    std::vector<uint16_t> mult(n);
    std::vector<uint8_t> valid(n);
    read_exact(f, keys.data(), 8 * n);
    read_exact(f, mult.data(), 2 * n);
    read_exact(f, valid.data(), n);
    std::fclose(f);
    return SDBG(k, std::move(keys), std::move(mult), std::move(valid));
}

struct Out {
    std::FILE *f;
    explicit Out(const char *path) : f(std::fopen(path, "wb")) {
        if (!f) die(std::string("cannot write ") + path);
    }
    void u64(uint64_t v) { if (std::fwrite(&v, 8, 1, f) != 1) die("write failed"); }
    void bytes(const void *p, size_t n) { if (n && std::fwrite(p, 1, n, f) != n) die("write failed"); }
    void close() { if (std::fclose(f) != 0) die("write failed"); }
};

int run(int argc, char **argv) {
    if (argc != 8) die("usage: ref_cf run GRAPH RESULT threshold low_abundance max_length min_length");
    SDBG graph = read_graph(argv[2]);
    Settings settings;
    settings.threads = 1;
    settings.sdbg = &graph;
    settings.cycle_finder_settings.threshold_multiplicity = std::strtoull(argv[4], nullptr, 10);
    settings.cycle_finder_settings.low_abundance = std::atoi(argv[5]) != 0;
    settings.cycle_finder_settings.cycle_max_length = std::atoi(argv[6]);
    settings.cycle_finder_settings.cycle_min_length = std::atoi(argv[7]);

    CycleFinder finder(settings);  // the constructor runs the whole search

    std::cout << "ref_cf: second ChunkStartNodes" << std::endl;
    std::map<int, std::vector<uint64_t>, std::greater<int>> buckets;
    finder.ChunkStartNodes(buckets);
    std::cout.flush();

    Out out(argv[3]);
    out.u64(finder.results.size());
    for (const auto &entry : finder.results) {
        out.u64(entry.first);
        out.u64(entry.second.size());
        for (const auto &cycle : entry.second) {
            out.u64(cycle.size());
            out.bytes(cycle.data(), 8 * cycle.size());
        }
    }
    out.u64(buckets.size());
    for (const auto &b : buckets) {
        out.u64(uint64_t(int64_t(b.first)));
        out.u64(b.second.size());
        out.bytes(b.second.data(), 8 * b.second.size());
    }
    out.u64(graph.size());
    out.bytes(graph.valid_bytes().data(), graph.size());
    out.close();
    return 0;
}

int neighbors(int argc, char **argv) {
    if (argc != 4) die("usage: ref_cf neighbors GRAPH RESULT");
    SDBG graph = read_graph(argv[2]);
    Out out(argv[3]);
    uint64_t buf[4];
    for (uint64_t e = 0; e < graph.size(); ++e) {
        int n = graph.OutgoingEdges(e, buf);
        if (n != graph.EdgeOutdegree(e) || (n == 0) != graph.EdgeOutdegreeZero(e)) die("out-degree mismatch");
        out.u64(n);
        out.bytes(buf, 8 * n);
        n = graph.IncomingEdges(e, buf);
        if (n != graph.EdgeIndegree(e)) die("in-degree mismatch");
        out.u64(n);
        out.bytes(buf, 8 * n);
    }
    out.close();
    return 0;
}

}  // namespace

int main(int argc, char **argv) {
    try {
        if (argc >= 2 && std::strcmp(argv[1], "run") == 0) return run(argc, argv);
        if (argc >= 2 && std::strcmp(argv[1], "neighbors") == 0) return neighbors(argc, argv);
    } catch (const std::exception &e) {
        die(e.what());
    }
    die("usage: ref_cf run|neighbors GRAPH RESULT [settings]");
    return 2;
}
