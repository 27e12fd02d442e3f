// fasta_split.h — where a FASTA file may be cut into a rank's part.
//
// A record starts at a line whose first byte is '>'; a '>' anywhere else (inside a header)
// means nothing. A part of a file is [cut(S*part/n), cut(S*(part+1)/n)), where cut(pos) is the
// first such line start at or after pos, so every record lies whole in exactly one part.
//
// Self-contained (no HIP header needed), so a plain host compiler can build it alone.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

namespace mcaat {

// Index of the first header line start in the window w[0, n), or n when it holds none.
// line_start says whether w[0] begins a line (the byte before the window is '\n', or the
// window begins the file); every other index begins a line when the byte before it is '\n'.
inline size_t fasta_first_header(const uint8_t *w, size_t n, bool line_start) {
    size_t i = 0;
    while (i < n) {
        const void *p = memchr(w + i, '>', n - i);
        if (!p) return n;
        i = (size_t)(static_cast<const uint8_t *>(p) - w);
        if (i == 0 ? line_start : w[i - 1] == '\n') return i;
        ++i;
    }
    return n;
}

}  // namespace mcaat
