/*
 * parallel_hashmap/phmap.h — TEST INFRASTRUCTURE ONLY. A stand-in written for this project so
 * that the reference's cycle_finder.cpp compiles (`make -C oracle ref`). CycleFinder uses
 * phmap::flat_hash_set only for membership (find / insert / clear) in DepthLevelSearch, never
 * for iteration, so the standard set gives the same results.
 */
#ifndef MCAAT_REF_STANDIN_PHMAP_H
#define MCAAT_REF_STANDIN_PHMAP_H

#include <unordered_set>

namespace phmap {
template <class T> using flat_hash_set = std::unordered_set<T>;
}

#endif
