// partition_spec.h -- RAxML-style partition files (PhyloSuperTree::readPartitionRaxml, phylosupertree.cpp:150-266) and the
// position lists of Alignment::extractSites (extractSiteID / convert_range, alignment.cpp:2122-2200).  Plain C++, no
// device, no other header of this library: tools/asan_partition_spec.sh runs it under ASan + UBSan on its own.
//
//     MODEL, name = 1-100, 250-400, 401-500\3
//
// One partition per non-blank line.  The model field ends at the first comma OUTSIDE braces and is kept verbatim -- it is a
// string in this driver's own -m syntax, which carries commas inside its braces (GTR{1.5,2.4,..}+F{..}+G4{0.8}); the
// reference's RAxML keywords (DNA, BIN, MULTI, a trailing F / X) are not translated.  The name ends at '='.  Positions
// are 1-based and inclusive, separated by commas and / or blanks: a, a-b, or a-b\s (every s-th site from a); blanks
// around '-' and '\' are allowed.  Sites come out in the order written, duplicates included, as extractSiteID gives them.
// Refused (std::runtime_error): no comma after the model, no '=', an empty model or name, something that is not a
// position, a position < 1 or beyond the alignment, a range whose end lies before its start, a step < 1, a partition
// without a site, a file without a partition.
#pragma once
#include <stdint.h>

#include <stdexcept>
#include <string>
#include <vector>

namespace iqhost {

struct PartitionSpec {
    std::string model, name;
    std::vector<int> sites;   // 0-based
};

namespace partition_detail {

inline std::string trim(const std::string &s) {
    size_t a = 0, b = s.size();
    while (a < b && (s[a] == ' ' || s[a] == '\t' || s[a] == '\r' || s[a] == '\n')) a++;
    while (b > a && (s[b - 1] == ' ' || s[b - 1] == '\t' || s[b - 1] == '\r' || s[b - 1] == '\n')) b--;
    return s.substr(a, b - a);
}

inline bool isBlank(char c) { return c == ' ' || c == '\t' || c == '\r' || c == ','; }

// a decimal number of at most 9 digits at s[i]; false when there is none
inline bool readInt(const std::string &s, size_t &i, long &out) {
    const size_t start = i;
    long v = 0;
    while (i < s.size() && s[i] >= '0' && s[i] <= '9') {
        if (i - start >= 9) throw std::runtime_error("partition file: position too large in \"" + s + "\"");
        v = v * 10 + (s[i] - '0');
        i++;
    }
    out = v;
    return i > start;
}

inline void skipSpaces(const std::string &s, size_t &i) {
    while (i < s.size() && (s[i] == ' ' || s[i] == '\t' || s[i] == '\r')) i++;
}

}  // namespace partition_detail

// "1-100, 250-400 401-500\3" -> 0-based sites of an alignment of nsite sites
inline std::vector<int> parsePositions(const std::string &spec, int nsite) {
    using namespace partition_detail;
    std::vector<int> sites;
    size_t i = 0;
    for (;;) {
        while (i < spec.size() && isBlank(spec[i])) i++;
        if (i >= spec.size()) break;
        long lo, hi, step = 1;
        if (!readInt(spec, i, lo)) throw std::runtime_error("partition file: expecting a position in \"" + spec + "\"");
        hi = lo;
        size_t j = i;
        skipSpaces(spec, j);
        if (j < spec.size() && spec[j] == '-') {
            j++;
            skipSpaces(spec, j);
            if (!readInt(spec, j, hi)) throw std::runtime_error("partition file: expecting the end of a range in \"" + spec + "\"");
            i = j;
            skipSpaces(spec, j);
            if (j < spec.size() && spec[j] == '\\') {
                j++;
                skipSpaces(spec, j);
                if (!readInt(spec, j, step)) throw std::runtime_error("partition file: expecting a step in \"" + spec + "\"");
                i = j;
            }
        }
        if (i < spec.size() && !isBlank(spec[i])) throw std::runtime_error("partition file: bad range in \"" + spec + "\"");
        if (lo < 1 || hi > nsite) throw std::runtime_error("partition file: position outside the alignment in \"" + spec + "\"");
        if (lo > hi) throw std::runtime_error("partition file: empty range in \"" + spec + "\"");
        if (step < 1) throw std::runtime_error("partition file: step < 1 in \"" + spec + "\"");
        for (long s = lo - 1; s < hi; s += step) sites.push_back((int)s);
    }
    if (sites.empty()) throw std::runtime_error("partition file: partition without a site");
    return sites;
}

inline std::vector<PartitionSpec> parsePartitionFile(const std::string &text, int nsite) {
    using namespace partition_detail;
    std::vector<PartitionSpec> parts;
    size_t pos = 0;
    while (pos <= text.size()) {
        size_t eol = text.find('\n', pos);
        if (eol == std::string::npos) eol = text.size();
        const std::string line = trim(text.substr(pos, eol - pos));
        pos = eol + 1;
        if (line.empty()) continue;
        int depth = 0;
        size_t comma = std::string::npos;
        for (size_t k = 0; k < line.size(); k++) {
            if (line[k] == '{') depth++;
            else if (line[k] == '}') depth--;
            else if (line[k] == ',' && depth == 0) { comma = k; break; }
        }
        if (comma == std::string::npos) throw std::runtime_error("partition file: no ',' after the model in \"" + line + "\"");
        const size_t eq = line.find('=', comma + 1);
        if (eq == std::string::npos) throw std::runtime_error("partition file: no '=' in \"" + line + "\"");
        PartitionSpec p;
        p.model = trim(line.substr(0, comma));
        p.name = trim(line.substr(comma + 1, eq - comma - 1));
        if (p.model.empty()) throw std::runtime_error("partition file: no model in \"" + line + "\"");
        if (p.name.empty()) throw std::runtime_error("partition file: no partition name in \"" + line + "\"");
        p.sites = parsePositions(line.substr(eq + 1), nsite);
        parts.push_back(std::move(p));
    }
    if (parts.empty()) throw std::runtime_error("partition file: no partition");
    return parts;
}

// the chosen columns of every sequence, in order (Alignment::extractSites); every sequence must have nsite characters
inline std::vector<std::string> extractSites(const std::vector<std::string> &sequences, const std::vector<int> &sites) {
    std::vector<std::string> out(sequences.size());
    for (size_t t = 0; t < sequences.size(); t++) {
        out[t].reserve(sites.size());
        for (int s : sites) {
            if (s < 0 || (size_t)s >= sequences[t].size()) throw std::runtime_error("partition file: site beyond a sequence");
            out[t].push_back(sequences[t][(size_t)s]);
        }
    }
    return out;
}

}  // namespace iqhost
