// Stand-alone driver of iq-tree_amd/host/partition_spec.h for tools/asan_partition_spec.sh (AddressSanitizer + UBSan on the
// CPU): well-formed and broken partition files, position lists at the edges of the alignment, site extraction, and random
// byte strings thrown at both parsers.
#include <stdio.h>
#include <stdlib.h>

#include <random>

#include "../iq-tree_amd/host/partition_spec.h"

static int failures = 0;
#define EXPECT(cond)                                                     \
    do {                                                                 \
        if (!(cond)) {                                                   \
            fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); \
            failures++;                                                  \
        }                                                                \
    } while (0)

template <typename F>
static bool throws(F &&f) {
    try {
        f();
    } catch (const std::runtime_error &) {
        return true;
    }
    return false;
}

int main() {
    using namespace iqhost;
    const std::string text =
        "GTR{1.5,2.4,1.8,1.9,2.8}+F{0.25,0.26,0.25,0.24}+G4{0.8}, gene1 = 1-100, 250-400\n"
        "\n"
        "  JC ,  gene 2=101 - 249\r\n"
        "LG+G4{0.5}, third = 401-500\\3 , 402-500 \\ 3  7\n";
    std::vector<PartitionSpec> parts = parsePartitionFile(text, 500);
    EXPECT(parts.size() == 3);
    EXPECT(parts[0].model == "GTR{1.5,2.4,1.8,1.9,2.8}+F{0.25,0.26,0.25,0.24}+G4{0.8}" && parts[0].name == "gene1");
    EXPECT(parts[0].sites.size() == 100 + 151 && parts[0].sites.front() == 0 && parts[0].sites[100] == 249 && parts[0].sites.back() == 399);
    EXPECT(parts[1].model == "JC" && parts[1].name == "gene 2" && parts[1].sites.size() == 149 && parts[1].sites.back() == 248);
    EXPECT(parts[2].sites.size() == 34 + 33 + 1 && parts[2].sites[0] == 400 && parts[2].sites[1] == 403 && parts[2].sites[34] == 401 &&
           parts[2].sites.back() == 6);
    EXPECT(parsePositions("500", 500) == std::vector<int>{499});
    EXPECT(parsePositions("1-1", 1) == std::vector<int>{0});
    const char *broken[] = {"", "\n\n", "JC gene = 1-10", "JC, gene 1-10", "JC, = 1-10", ", gene = 1-10", "JC, gene =", "JC, gene = ,",
                            "JC, gene = 0-10", "JC, gene = 1-501", "JC, gene = 10-1", "JC, gene = 1-10\\0", "JC, gene = 1-", "JC, gene = a-b",
                            "JC, gene = 1-10\\", "JC, gene = 1--2", "JC, gene = 1-10x", "JC, gene = 99999999999", "GTR{1,2, gene = 1-10",
                            "JC, gene = -3", "JC, gene = 3\\2"};
    for (const char *b : broken) EXPECT(throws([&] { parsePartitionFile(b, 500); }));
    const std::vector<std::string> seqs = {"ACGTACGTAC", "TTTTTGGGGG"};
    const std::vector<std::string> ex = extractSites(seqs, parsePositions("1-10\\3 2", 10));
    EXPECT(ex[0] == "ATGCC" && ex[1] == "TTGGT");
    EXPECT(throws([&] { extractSites(seqs, {10}); }));
    EXPECT(throws([&] { extractSites(seqs, {-1}); }));
    // random strings over the alphabet of the format: either a parse or a std::runtime_error, never anything else
    std::mt19937_64 gen(11);
    const std::string alphabet = "0123456789-\\,= {}\nJC+G\t";
    int parsed = 0;
    for (int k = 0; k < 20000; k++) {
        std::string s;
        const int len = (int)(gen() % 40);
        for (int i = 0; i < len; i++) s.push_back(alphabet[gen() % alphabet.size()]);
        try {
            parsed += (int)parsePartitionFile("JC, g = " + s, 1000).size();
        } catch (const std::runtime_error &) {
        }
        try {
            parsed += (int)parsePartitionFile(s, 50).size();
        } catch (const std::runtime_error &) {
        }
    }
    EXPECT(parsed > 0);
    if (failures) {
        fprintf(stderr, "%d check(s) failed\n", failures);
        return 1;
    }
    printf("partition_spec.h: all checks passed (%d random partitions parsed)\n", parsed);
    return 0;
}
