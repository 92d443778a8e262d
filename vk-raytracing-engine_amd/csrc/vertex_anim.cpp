// vertex_anim.cpp -- the argument rules of the vertex-animation entry points (vertex_anim.h): host-only, no HIP type.
#include "vertex_anim.h"

#include <cmath>
#include <cstdarg>
#include <cstdio>

namespace vkrt {

namespace {

int refuse(std::string& err, const char* fmt, ...)
{
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  err = buf;
  return VKRT_ERR_INVALID_ARGUMENT;
}

// NULL, then device memory that is not `align`-byte aligned
int check_source(const char* who, const char* name, const float* p, uint32_t memory, unsigned align, std::string& err)
{
  if(!p)
    return refuse(err, "%s: %s is NULL", who, name);
  if(memory != VKRT_MEMORY_HOST && ((uintptr_t)p & (align - 1u)) != 0)
    return refuse(err, "%s: %s %p is not %u-byte aligned", who, name, (const void*)p, align);
  return VKRT_OK;
}

int check_index(const char* who, const char* what, uint32_t index, size_t count, std::string& err)
{
  if(index >= count)
    return refuse(err, "%s: %s %u outside the scene's %zu %ss", who, what, index, count, what);
  return VKRT_OK;
}

// outside the scene, then empty
int check_bound_range(const char* who, uint32_t first, uint32_t count, size_t vertexCount, std::string& err)
{
  if(const int rc = check_vertex_range(who, first, count, vertexCount, err); rc != VKRT_OK)
    return rc;
  return count ? VKRT_OK : refuse(err, "%s: count is 0", who);
}

}  // namespace

int RangeSet::overlapping(uint32_t first, uint32_t count) const
{
  for(size_t j = 0; j < size; j++)
  {
    const VertexRange& a = (*this)[j];
    if(first < (uint64_t)a.first + a.count && a.first < (uint64_t)first + count)
      return (int)j;
  }
  return -1;
}

bool RangeSet::contains(size_t j, uint32_t first, uint32_t count) const
{
  const VertexRange& a = (*this)[j];
  return first >= a.first && (uint64_t)first + count <= (uint64_t)a.first + a.count;
}

int check_memory(const char* who, uint32_t memory, std::string& err)
{
  if(memory != VKRT_MEMORY_HOST && memory != VKRT_MEMORY_DEVICE)
    return refuse(err, "%s: memory %u is neither VKRT_MEMORY_HOST nor VKRT_MEMORY_DEVICE", who, memory);
  return VKRT_OK;
}

int check_vertex_range(const char* who, uint32_t first, uint32_t count, size_t vertexCount, std::string& err)
{
  if((uint64_t)first + count > vertexCount)
    return refuse(err, "%s: vertices [%u, %llu) outside the scene's %zu vertices", who, first, (unsigned long long)first + count, vertexCount);
  return VKRT_OK;
}

size_t first_non_finite(const float* a, size_t n)
{
  size_t i = 0;
  while(i < n && std::isfinite(a[i]))
    i++;
  return i;
}

// ---- vkrt_scene_update_vertices ----------------------------------------------------------------------------------------------------------
int check_update_desc(const vkrt_vertex_update* u, std::string& err)
{
  const char* who = "vkrt_scene_update_vertices";
  if(!u)
    return refuse(err, "%s: update is NULL", who);
  if(u->struct_size < sizeof(vkrt_vertex_update))
    return refuse(err, "%s: vkrt_vertex_update.struct_size %u < %zu (ABI mismatch)", who, u->struct_size, sizeof(vkrt_vertex_update));
  return check_memory(who, u->memory, err);
}

int check_update_range(const vkrt_vertex_update& u, size_t vertexCount, std::string& err)
{
  const char* who = "vkrt_scene_update_vertices";
  if(const int rc = check_vertex_range(who, u.first, u.count, vertexCount, err); rc != VKRT_OK)
    return rc;
  // the rule of vkrt_scene_create, checked for the whole range before anything changes
  if(u.memory == VKRT_MEMORY_HOST && u.positions)
    if(const size_t n = 3 * (size_t)u.count, i = first_non_finite(u.positions, n); i < n)
      return refuse(err, "%s: positions[%zu] (vertex %zu) is not finite", who, i, (size_t)u.first + i / 3);
  return VKRT_OK;
}

// ---- vkrt_scene_add_skin / vkrt_scene_skin_vertices --------------------------------------------------------------------------------------
int check_skin_desc(const vkrt_skin_desc* k, std::string& err)
{
  const char* who = "vkrt_scene_add_skin";
  if(!k)
    return refuse(err, "%s: desc is NULL", who);
  if(k->struct_size < sizeof(vkrt_skin_desc))
    return refuse(err, "%s: vkrt_skin_desc.struct_size %u < %zu (ABI mismatch)", who, k->struct_size, sizeof(vkrt_skin_desc));
  if(k->joint_count == 0 || k->joint_count > 65536u)
    return refuse(err, "%s: joint_count %u outside 1..65536", who, k->joint_count);
  const size_t n = 4 * (size_t)k->count;
  if(n && !k->joints)
    return refuse(err, "%s: joints is NULL", who);
  if(n && !k->weights)
    return refuse(err, "%s: weights is NULL", who);
  // the gather of k_skin is bounded here: no later call looks at an index again
  for(size_t i = 0; i < n; i++)
    if(k->joints[i] >= k->joint_count)
      return refuse(err, "%s: joints[%zu] (vertex %zu) is %u, joint_count is %u", who, i, (size_t)k->first + i / 4, (unsigned)k->joints[i], k->joint_count);
  if(const size_t i = first_non_finite(k->weights, n); i < n)
    return refuse(err, "%s: weights[%zu] (vertex %zu) is not finite", who, i, (size_t)k->first + i / 4);
  return VKRT_OK;
}

int check_skin_range(const vkrt_skin_desc& k, size_t vertexCount, const RangeSet& skins, const RangeSet& morphs, std::string& err)
{
  const char* who = "vkrt_scene_add_skin";
  if(const int rc = check_bound_range(who, k.first, k.count, vertexCount, err); rc != VKRT_OK)
    return rc;
  const uint32_t end = k.first + k.count;
  if(const int j = skins.overlapping(k.first, k.count); j >= 0)
    return refuse(err, "%s: vertices [%u, %u) overlap skin %zu's [%u, %u)", who, k.first, end, (size_t)j, skins[j].first, skins[j].first + skins[j].count);
  // (skins come first: a morph inside a skin's range captured its base from that skin's bind pose)
  if(const int j = morphs.overlapping(k.first, k.count); j >= 0)
    return refuse(err, "%s: vertices [%u, %u) overlap morph %zu's [%u, %u): add skins before morphs", who, k.first, end, (size_t)j, morphs[j].first,
                  morphs[j].first + morphs[j].count);
  return VKRT_OK;
}

int check_skin_index(uint32_t skin, size_t skinCount, std::string& err) { return check_index("vkrt_scene_skin_vertices", "skin", skin, skinCount, err); }

int check_joint_matrices(const float* jointMatrices, uint32_t memory, uint32_t jointCount, std::string& err)
{
  const char* who = "vkrt_scene_skin_vertices";
  if(const int rc = check_source(who, "joint_matrices", jointMatrices, memory, 16, err); rc != VKRT_OK)
    return rc;
  if(memory == VKRT_MEMORY_HOST)
    if(const size_t n = (size_t)jointCount * 16, i = first_non_finite(jointMatrices, n); i < n)
      return refuse(err, "%s: joint_matrices[%zu] (joint %zu) is not finite", who, i, i / 16);
  return VKRT_OK;
}

// ---- vkrt_scene_add_morph / vkrt_scene_morph_vertices ------------------------------------------------------------------------------------
int check_morph_desc(const vkrt_morph_desc* m, std::string& err)
{
  const char* who = "vkrt_scene_add_morph";
  if(!m)
    return refuse(err, "%s: desc is NULL", who);
  if(m->struct_size < sizeof(vkrt_morph_desc))
    return refuse(err, "%s: vkrt_morph_desc.struct_size %u < %zu (ABI mismatch)", who, m->struct_size, sizeof(vkrt_morph_desc));
  if(m->target_count == 0 || m->target_count > VKRT_MORPH_TARGETS_MAX)
    return refuse(err, "%s: target_count %u outside 1..%u", who, m->target_count, (unsigned)VKRT_MORPH_TARGETS_MAX);
  if(!m->position_deltas && !m->normal_deltas && !m->tangent_deltas)
    return refuse(err, "%s: position_deltas, normal_deltas and tangent_deltas are all NULL", who);
  const size_t n = m->count, floats = (size_t)m->target_count * n * 3;
  const float* const deltas[3] = {m->position_deltas, m->normal_deltas, m->tangent_deltas};
  const char* const names[3] = {"position_deltas", "normal_deltas", "tangent_deltas"};
  for(int a = 0; a < 3; a++)
    if(deltas[a])
      if(const size_t i = first_non_finite(deltas[a], floats); i < floats)
        return refuse(err, "%s: %s[%zu] (target %zu, vertex %zu) is not finite", who, names[a], i, i / (3 * n), (size_t)m->first + i / 3 % n);
  return VKRT_OK;
}

int check_morph_range(const vkrt_morph_desc& m, size_t vertexCount, const RangeSet& skins, const RangeSet& morphs, int& inSkin, std::string& err)
{
  const char* who = "vkrt_scene_add_morph";
  if(const int rc = check_bound_range(who, m.first, m.count, vertexCount, err); rc != VKRT_OK)
    return rc;
  const uint32_t end = m.first + m.count;
  if(const int j = morphs.overlapping(m.first, m.count); j >= 0)
    return refuse(err, "%s: vertices [%u, %u) overlap morph %zu's [%u, %u)", who, m.first, end, (size_t)j, morphs[j].first, morphs[j].first + morphs[j].count);
  // inside one skin or clear of all of them
  inSkin = skins.overlapping(m.first, m.count);
  if(inSkin >= 0 && !skins.contains(inSkin, m.first, m.count))
    return refuse(err, "%s: vertices [%u, %u) straddle the boundary of skin %zu's [%u, %u): a morph lies inside one skin or outside all", who, m.first, end,
                  (size_t)inSkin, skins[inSkin].first, skins[inSkin].first + skins[inSkin].count);
  return VKRT_OK;
}

int check_morph_index(uint32_t morph, size_t morphCount, std::string& err) { return check_index("vkrt_scene_morph_vertices", "morph", morph, morphCount, err); }

int check_morph_weights(const float* weights, uint32_t memory, uint32_t targetCount, std::string& err)
{
  const char* who = "vkrt_scene_morph_vertices";
  if(const int rc = check_source(who, "weights", weights, memory, 4, err); rc != VKRT_OK)
    return rc;
  if(memory == VKRT_MEMORY_HOST)
    if(const size_t i = first_non_finite(weights, targetCount); i < targetCount)
      return refuse(err, "%s: weights[%zu] is not finite", who, i);
  return VKRT_OK;
}

}  // namespace vkrt
