// Host-only witness of the weight layouts: runs the three pack functions sgpr_create uploads from (sgpr_model.hpp) on a
// blob file and writes every buffer + every offset / scalar to a directory.  tests/test_model_pack_host.py compares them
// with tests/golden/model_pack.json.
//   pack_dump <blob file> <num_labels> <filters_1> <filters_2> <filters_3> <tensor_neurons> <bottle_neck_neurons> <out dir>
#include <stdio.h>
#include <stdlib.h>

#include <string>
#include <vector>

#include "sgpr_model.hpp"

using namespace sgpr;

static std::string g_dir;
static FILE* g_meta = nullptr;

static void dump_file(const char* name, const void* p, size_t bytes) {
    FILE* f = fopen((g_dir + "/" + name).c_str(), "wb");
    if (!f || fwrite(p, 1, bytes, f) != bytes) {
        fprintf(stderr, "pack_dump: cannot write %s\n", name);
        exit(2);
    }
    fclose(f);
}
static void meta_z(const char* name, const size_t* v, int n) {
    fprintf(g_meta, "%s", name);
    for (int i = 0; i < n; ++i) fprintf(g_meta, " %zu", v[i]);
    fprintf(g_meta, "\n");
}
static void meta_i(const char* name, const int* v, int n) {
    fprintf(g_meta, "%s", name);
    for (int i = 0; i < n; ++i) fprintf(g_meta, " %d", v[i]);
    fprintf(g_meta, "\n");
}
static void meta_f(const char* name, float v) { fprintf(g_meta, "%s %a\n", name, (double)v); }
static void meta_head(const std::string& prefix, const HeadRange& hr) {
    meta_f((prefix + ".head_scale").c_str(), hr.scale);
    meta_f((prefix + ".head_nl2e").c_str(), hr.nl2e);
    meta_i((prefix + ".head_f16").c_str(), &hr.f16_ok, 1);
}

int main(int argc, char** argv) {
    if (argc != 9) {
        fprintf(stderr, "usage: pack_dump blob L f1 f2 f3 T B outdir\n");
        return 2;
    }
    const sgpr_dims d = {atoi(argv[2]), atoi(argv[3]), atoi(argv[4]), atoi(argv[5]), atoi(argv[6]), atoi(argv[7])};
    g_dir = argv[8];
    if (!dims_supported(&d) && !dims_generic(&d)) {
        fprintf(stderr, "pack_dump: dims not served\n");
        return 2;
    }
    std::vector<float> blob(weights_count(&d));
    FILE* f = fopen(argv[1], "rb");
    if (!f || fread(blob.data(), sizeof(float), blob.size(), f) != blob.size() || fgetc(f) != EOF) {
        fprintf(stderr, "pack_dump: %s does not hold %zu floats\n", argv[1], blob.size());
        return 2;
    }
    fclose(f);
    g_meta = fopen((g_dir + "/meta.txt").c_str(), "w");
    if (!g_meta) return 2;

    const bool generic_only = !dims_supported(&d);
    const FoldedNet net = fold_model(blob.data(), &d);
    if (!generic_only) {
        const PackedBuilt pb = pack_built(net);
        dump_file("built.bin", pb.blob.data(), pb.blob.size() * sizeof(float));
        const size_t n = pb.blob.size();
        meta_z("built.floats", &n, 1);
        meta_z("built.off_wf", pb.off_wf, 7);
        meta_z("built.off_tb", pb.off_tb, 7);
        meta_z("built.off_wb", pb.off_wb, 7);
        meta_z("built.off_wh", pb.off_wh, 7);
        meta_i("built.kp", pb.kp, 6);
        meta_i("built.cout", pb.cout, 6);
        meta_z("built.off_tail", pb.off_tail, kTails);
        meta_z("built.off_ntwt", &pb.off_ntwt, 1);
        meta_z("built.off_semtab", &pb.off_semtab, 1);
        const int ok16 = pb.f16_ok ? 1 : 0;
        meta_i("built.f16_ok", &ok16, 1);
        meta_head("built", pb.head);
    }
    {
        const PackedGeneric pg = pack_generic(net);
        dump_file("generic.bin", pg.blob.data(), pg.blob.size() * sizeof(float));
        const size_t n = pg.blob.size();
        meta_z("generic.floats", &n, 1);
        const int dd[6] = {d.num_labels, d.filters_1, d.filters_2, d.filters_3, d.tensor_neurons, d.bottle_neck_neurons};
        meta_i("generic.dims", dd, 6);
        meta_i("generic.cmax", &pg.cmax, 1);
        meta_i("generic.cin", pg.cin, 6);
        meta_i("generic.cout", pg.cout, 6);
        meta_z("generic.off_wa", pg.off_wa, 6);
        meta_z("generic.off_wb", pg.off_wb, 6);
        meta_z("generic.off_tb", pg.off_tb, 6);
        meta_z("generic.off_wend", &pg.off_wend, 1);
        meta_z("generic.off_tend", &pg.off_tend, 1);
        meta_z("generic.off_tail", pg.off_tail, kTails);
        meta_head("generic", pg.head);
    }
    {
        const PackedWide pw = pack_wide(net, generic_only);
        const int ok = pw.ok ? 1 : 0;
        meta_i("wide.ok", &ok, 1);
        if (pw.ok) {
            dump_file("wide_planes.bin", pw.planes.data(), pw.planes.size() * sizeof(unsigned short));
            dump_file("wide_tbs.bin", pw.tbs.data(), pw.tbs.size() * sizeof(float));
            const size_t np = pw.planes.size(), nt = pw.tbs.size();
            meta_z("wide.planes", &np, 1);
            meta_z("wide.tbs", &nt, 1);
            meta_z("wide.plane_bytes", &pw.plane_bytes, 1);
            meta_i("wide.cinP", pw.cinP, 6);
            meta_i("wide.coutP", pw.coutP, 6);
            meta_i("wide.F3P", &pw.F3P, 1);
            meta_z("wide.off_wh", pw.off_wh, 7);
            meta_z("wide.off_tbp", pw.off_tbp, 7);
        }
    }
    fclose(g_meta);
    return 0;
}
