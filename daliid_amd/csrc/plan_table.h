// plan_table.h -- what the net plans (resnet_plan.hip, vit_plan.hip) share: the table of named tensors in the flat fp32 parameter / buffer
// storages, and the table of named tensors in the byte arena, whose offsets become pointers at bind().
#pragma once
#include "common.h"
#include <cstdio>
#include <initializer_list>
#include <string>
#include <vector>

namespace dali {

struct TensorInfo { std::string name; int64_t offset, numel; int shape[4]; int ndim; };
// A named tensor of the arena.  offset >= 0: reserved, bind_arena sets *slot = arena + offset.  offset -1: a view, a name for storage that lies
// inside a reserved tensor; whoever aliases it sets the slot.  A slot that is (still) null: this plan does not hold the tensor.
struct ArenaEntry { std::string name; void** slot; int64_t offset; size_t bytes; };

struct PlanTable {
    std::vector<TensorInfo> params, buffers;
    int64_t param_elems = 0, buffer_elems = 0;
    size_t arena_bytes = 0;
    std::vector<ArenaEntry> arena_entries;               // every arena tensor is declared once, here: name, pointer and size

    // appends a tensor to `v` (params with param_elems, buffers with buffer_elems); returns its element offset
    static int64_t add_tensor(std::vector<TensorInfo>& v, int64_t& total, const std::string& name, std::initializer_list<int> shape) {
        TensorInfo t;
        t.name = name;
        t.ndim = (int)shape.size();
        t.numel = 1;
        int i = 0;
        for (int s : shape) { t.shape[i++] = s; t.numel *= s; }
        for (; i < 4; ++i) t.shape[i] = 1;
        t.offset = total;
        total += (t.numel + 63) / 64 * 64;          // 256-byte aligned segments
        v.push_back(t);
        return t.offset;
    }
    int64_t add_param(const std::string& name, std::initializer_list<int> shape) { return add_tensor(params, param_elems, name, shape); }
    int64_t add_buffer(const std::string& name, std::initializer_list<int> shape) { return add_tensor(buffers, buffer_elems, name, shape); }

    // `bytes` of the arena (256-byte aligned) for ptr, which bind_arena sets
    template <class T>
    void reserve(const std::string& name, T*& ptr, size_t bytes) {
        arena_entries.push_back({name, reinterpret_cast<void**>(&ptr), (int64_t)arena_bytes, bytes});
        arena_bytes = align_up(arena_bytes + bytes, 256);
    }
    template <class T>
    void view(const std::string& name, T*& ptr, size_t bytes) { arena_entries.push_back({name, reinterpret_cast<void**>(&ptr), -1, bytes}); }
    void bind_arena(char* arena) { for (auto& e : arena_entries) if (e.offset >= 0) *e.slot = arena + e.offset; }

    // the bodies of dali_*_sizes and dali_*_tensor_info
    int sizes(int feat, int64_t* param_elems_out, int64_t* buffer_elems_out, int64_t* arena_bytes_out, int* feat_dim, int* n_params, int* n_buffers) const {
        if (param_elems_out) *param_elems_out = param_elems;
        if (buffer_elems_out) *buffer_elems_out = buffer_elems;
        if (arena_bytes_out) *arena_bytes_out = (int64_t)arena_bytes;
        if (feat_dim) *feat_dim = feat;
        if (n_params) *n_params = (int)params.size();
        if (n_buffers) *n_buffers = (int)buffers.size();
        return DALI_OK;
    }
    int tensor_info(const char* who, int kind, int index, char* name, int name_cap, int64_t* offset, int64_t* numel, int* shape4, int* ndim) const {
        DALI_REQUIRE(name && offset && numel && shape4 && ndim, "%s: null argument", who);
        const auto& v = kind == 0 ? params : buffers;
        DALI_REQUIRE(index >= 0 && index < (int)v.size(), "%s: index %d out of range", who, index);
        const TensorInfo& t = v[index];
        snprintf(name, name_cap, "%s", t.name.c_str());
        *offset = t.offset; *numel = t.numel; *ndim = t.ndim;
        for (int i = 0; i < 4; ++i) shape4[i] = t.shape[i];
        return DALI_OK;
    }
    // the bodies of dali_*_debug_tensor and dali_debug_*_arena_entry
    int arena_tensor(const char* who, const char* name, void** ptr, int64_t* bytes) const {
        for (const ArenaEntry& e : arena_entries)
            if (e.name == name && *e.slot) { *ptr = *e.slot; *bytes = (int64_t)e.bytes; return DALI_OK; }
        set_error("%s: unknown tensor '%s', or one this plan does not hold", who, name);
        return DALI_ERR_INVALID;
    }
    int arena_entry(const char* who, int index, char* name, int name_cap, int64_t* offset, int64_t* bytes, int* reserved) const {
        DALI_REQUIRE(name && offset && bytes && reserved, "%s: null argument", who);
        DALI_REQUIRE(index >= 0 && index < (int)arena_entries.size(), "%s: index %d out of range", who, index);
        const ArenaEntry& e = arena_entries[index];
        snprintf(name, name_cap, "%s", e.name.c_str());
        *offset = e.offset; *bytes = (int64_t)e.bytes; *reserved = e.offset >= 0;
        return DALI_OK;
    }
};

}  // namespace dali
