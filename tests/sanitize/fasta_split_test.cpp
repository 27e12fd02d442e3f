// Where a FASTA file is cut into ranks' parts (mcaat_amd/csrc/fasta_split.h: fasta_first_header),
// built with AddressSanitizer and UndefinedBehaviorSanitizer by tests/test_fasta_split.py. On
// seeded FASTA texts (wrapped records, empty lines, '>' '@' '+' inside headers, LF and CRLF, a
// text with no header, a text that is one header without its newline) every start position is
// asked, as the file wrapper asks it: a window from pos - 1 that does not begin a line, and then
// cut into consecutive pieces of 1, 2, 3, 7, 64 and 4096 bytes with the line-start state carried
// from piece to piece. Every answer must equal a naive scan for the first '>' at or after pos
// that follows a '\n'. Each window is copied into a heap block of its exact size, so a read one
// byte before or past it is an AddressSanitizer report.
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <random>
#include <string>
#include <vector>

#include "../../mcaat_amd/csrc/fasta_split.h"

static std::string fasta_text(std::mt19937_64 &rng, int n_rec, bool crlf, bool final_newline) {
    const std::string nl = crlf ? "\r\n" : "\n";
    const int widths[] = {1, 7, 31, 32, 33, 60, 64, 80};
    std::string t = rng() % 2 ? "\n\n" : "";
    for (int i = 0; i < n_rec; ++i) {
        t += ">r" + std::to_string(i) + " x>y @z +w" + (rng() % 4 == 0 ? ">" : "") + nl;
        const size_t len = i % 5 == 0 ? 0 : rng() % 200;
        const size_t w = (size_t)widths[rng() % 8];
        for (size_t p = 0; p < len; p += w) {
            for (size_t j = p; j < len && j < p + w; ++j) t += "ACGTN"[rng() % 5];
            t += nl;
            if (rng() % 9 == 0) t += nl;
        }
    }
    if (!final_newline)
        while (!t.empty() && (t.back() == '\n' || t.back() == '\r')) t.pop_back();
    return t;
}

// first index >= pos that holds '>' right after a '\n' (pos >= 1); the size if none
static size_t naive(const std::string &t, size_t pos) {
    for (size_t i = pos; i < t.size(); ++i)
        if (t[i] == '>' && t[i - 1] == '\n') return i;
    return t.size();
}

// the wrapper's walk: pieces of at most `piece` bytes from pos - 1
static size_t walk(const std::string &t, size_t pos, size_t piece) {
    bool line_start = false;
    for (size_t at = pos - 1; at < t.size();) {
        const size_t n = std::min(piece, t.size() - at);
        std::vector<uint8_t> w(t.begin() + (long)at, t.begin() + (long)(at + n));  // exact-size heap block
        const size_t i = mcaat::fasta_first_header(w.data(), n, line_start);
        if (i > n) return (size_t)-1;
        if (i < n) return at + i;
        line_start = w[n - 1] == '\n';
        at += n;
    }
    return t.size();
}

int main() {
    std::mt19937_64 rng(11);
    std::vector<std::string> texts;
    for (int c = 0; c < 8; ++c) texts.push_back(fasta_text(rng, 3 + c * 4, c & 1, !(c & 2)));
    texts.push_back("ACGT\nAC>GT\n\nTT>\n");         // no header: '>' only inside lines
    texts.push_back(">only a header > with no newline");
    texts.push_back(">a\n>b\n>c\n\n>d");               // consecutive headers, a header as the last line
    texts.push_back(">a\r\nAC\r\n\r\n>b\r\nGT");      // CRLF, no final newline
    const size_t pieces[] = {1, 2, 3, 7, 64, 4096};
    size_t asked = 0;
    for (size_t ti = 0; ti < texts.size(); ++ti) {
        const std::string &t = texts[ti];
        for (size_t pos = 1; pos < t.size(); ++pos) {
            const size_t want = naive(t, pos);
            for (size_t piece : pieces) {
                const size_t got = walk(t, pos, piece);
                if (got != want) {
                    std::printf("FAIL text %zu pos %zu piece %zu: got %zu want %zu\n", ti, pos, piece, got, want);
                    return 1;
                }
                ++asked;
            }
        }
        // a window that begins a line (the start of the file), and an empty window
        std::vector<uint8_t> w(t.begin(), t.end());
        const size_t head = mcaat::fasta_first_header(w.data(), w.size(), true);
        const size_t want0 = !t.empty() && t[0] == '>' ? 0 : naive(t, 1);
        if (head != want0) {
            std::printf("FAIL text %zu from the start: got %zu want %zu\n", ti, head, want0);
            return 1;
        }
        if (mcaat::fasta_first_header(w.data(), 0, true) != 0) return 1;
    }
    std::printf("fasta_split ok: %zu positions\n", asked);
    return 0;
}
