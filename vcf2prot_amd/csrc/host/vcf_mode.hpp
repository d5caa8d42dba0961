// vcf_mode.hpp -- `v2p_harness vcf`: the product's command line (python -m vcf2prot_amd forwards its flags here); vcf_mode.cpp
#pragma once
#include <cstdint>
#include <string>
#include <vector>

struct VcfOptions {
    const char *vcf_path = nullptr, *fasta_path = nullptr, *outdir = nullptr;
    bool no_test = false, write_all = false, compressed = false, host_build = false, bgzf = false, stats = false, host_groups = false, device_tasks = false,
         device_tables = false, device_index = false, int_map = false, device_int_map = false, unique = false;
    uint64_t slice_bytes = 256ull << 20;     // --slice-kb K: slices of K KiB of FASTA text (tests: several slices out of a small file)
    std::vector<uint32_t> peptide_ks;        // --peptides K[,K...]
    bool tryptic = false;                    // --tryptic M,MIN,MAX
    uint32_t tryptic_missed = 0, tryptic_min = 0, tryptic_max = 0;
    bool carriers = false;                   // --carriers: {stem}.carriers.tsv beside every peptide file, and peptide_carriers_summary.tsv
    bool sources = false;                    // --sources: {stem}.sources.tsv beside every peptide file, and peptide_sources_summary.tsv
    bool find = false;                       // --find FILE: found_peptides.tsv and found_peptides.carriers.tsv
    std::vector<std::string> find_queries;   // the file's queries, in its order (read while the options are parsed)
};

// argv = {harness, "vcf", in.vcf, reference.fasta, outdir, flags...}; an argument that is no flag is ignored.  false: a combination that is
// refused -- the usage sentence is on stderr and *exit_code is what the process ends with
bool parse_vcf_options(int argc, char** argv, VcfOptions& opt, int* exit_code);

// 0, or throws a std::exception whose what() is the line the process ends with (exit status 101, as the reference's panics)
int vcf_mode(const VcfOptions& opt);
