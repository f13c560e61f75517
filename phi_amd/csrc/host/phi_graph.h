// phi_graph.h -- the graph behind the opaque phi_graph handle of include/phi_host.h: filled by the GFA reader
// (gfa_reader.cpp) or built from a phased VCF (vcf_reader.cpp); the accessors and the destructor are gfa_reader.cpp's.
#pragma once
#include <stdint.h>
#include <string>
#include <thread>
#include <vector>

struct GfaState;                                       // the text, its slices and the name table, while the walks are still text
struct phi_graph {
    GfaState *state = nullptr;
    bool name_index_ok = false;                        // every name is <prefix><number> and every W-line stands behind all S-lines
    std::vector<int32_t> num2id;                       // the name table's direct index (number -> segment id, -1: none)
    std::string prefix;
    std::vector<char> name_arena;                      // segment names, NUL-terminated, back to back
    std::vector<int64_t> name_off;
    std::vector<std::string> hap_names;
    char *seq_concat = nullptr;                        // malloc'd (not zero-filled: every byte is written)
    int32_t *walk_vtx = nullptr;
    std::vector<int64_t> seq_off, adj_off, walk_off;
    std::vector<int32_t> adj, topo_rank;
    int32_t n_seg = 0;
    GfaState *retired = nullptr;                       // the reader's state after the walks are resolved: only its mapping of the file is left
    std::thread reaper;                                // frees the line tables once the walks are resolved
    void let_state_go();
    ~phi_graph();
};
