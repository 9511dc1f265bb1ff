"""sdface-gan_amd: MI355X-native SDF + hash-grid renderer for SDFace-GAN.

Import name: ``sdface_gan_amd`` (see ``sdfr_loader.py`` at the repository root;
the directory name is not a valid Python identifier).

Drop-in surface (reference: im2scene/sdf/models/):
  Generator, VolumeFeatureRenderer, NGPSIRENGenerator, SirenGenerator,
  FCGenerator, LinearLayer, FiLMSiren, get_encoder      (sdf_model.py)
  GridEncoder, grid_encode                              (gridencoder/grid.py)
  SHEncoder, sh_encode                                  (shencoder/sphere_harmonics.py)
  generate_camera_params                                (sdf_utils.py:97-159)
  align_volume, extract_mesh_with_marching_cubes (+ marching_cubes, Mesh:
  HIP, csrc/mesh.hip), xyz2mesh                       (sdf_utils.py:164-223)
Beyond the reference: VolumeFeatureRenderer.query / Generator.query_field (the field at
arbitrary points, fused: sdfr_query_ngp_forward), cube_points, sdf_cube, world_to_network,
color_mesh (meshes from the field itself, vertex colours);
VolumeFeatureRenderer.query_gradient / Generator.query_field_gradient (the SDF's exact
gradient, fused: sdfr_query_ngp_grad), normal_mesh, eikonal_residual (vertex normals, the
eikonal check); VolumeFeatureRenderer.render_geometry / Generator.render_geometry -> Geometry
(the gradient along a render's own rays, normal / depth / xyz maps with the render's weights,
fused: sdfr_render_ngp_geometry); VolumeFeatureRenderer.render_surface /
Generator.render_surface -> Surface (per ray the SDF's first zero crossing, refined by
bisection, with the unit normal and the field's colour there, fused:
sdfr_render_ngp_surface / sdfr_render_siren_surface), shade_surface (a lit view of it);
extract_mesh_sparse / Generator.extract_mesh (the field's mesh at up to 1024^3 from
narrow-band 8^3 bricks, grown along the surface: csrc/mesh_sparse.hip), sparse_extract (the
generic driver), SparseVolume, cube_axis; mesh_components -> Components / keep_components
(a mesh's connected components labelled, measured, filtered and compacted on the GPU:
csrc/mesh_cc.hip, sdfr_mesh_cc_*; label_components, component_stats, sparse_mesh the pieces;
extract_mesh_sparse(components={"largest": 1}) filters before the host copy);
simplify_mesh -> Simplified (vertex clustering on a uniform grid, reproducible bit for bit:
csrc/mesh_simplify.hip, sdfr_mesh_simplify_*; simplify_grid its default grid;
extract_mesh_sparse(simplify=k) thins the mesh before the host copy);
smooth_mesh -> Smoothed (Laplacian / Taubin passes on an integer lattice, reproducible bit for
bit: csrc/mesh_smooth.hip, sdfr_mesh_smooth_*; smooth_lattice its default lattice;
mesh_boundary the valences and boundary flags; extract_mesh_sparse(smooth=n) smooths before
the host copy);
rasterize_mesh -> Raster (B views of a Mesh, nearest
triangle per pixel with depth and perspective-correct barycentrics, deterministic:
csrc/raster.hip, sdfr_mesh_raster), interpolate_vertex_attributes (sdfr_mesh_interpolate),
render_mesh (the Surface of a mesh), load_obj, subdivide_mesh; with them
Generator.forward(project_noise=True, mesh_path=...) (NoiseInjection.project_noise,
Decoder.reset_projected_noise), where the reference needs pytorch3d.
  SDFOptions, vol_render_opt                            (sdf_utils.py:447, training_utils.py:144)
Beyond the reference: GraphedGenerator (HIP-graph replay of the inference forward).
"""
from . import _lib  # noqa: F401
from .camera import generate_camera_params  # noqa: F401
from .encoders import GridEncoder, SHEncoder, grid_encode, sh_encode  # noqa: F401
from . import decoder_ops  # noqa: F401
from .generator import (Blur, Decoder, EqualLinear, FusedLeakyReLU, Generator,  # noqa: F401
                        MappingLinear, ModulatedConv2d, NoiseInjection, PixelNorm, StyledConv,
                        ToRGB, Upsample, fused_leaky_relu, make_kernel, upfirdn2d)
from .graphs import GraphedGenerator  # noqa: F401
from .mesh import (Components, Mesh, Simplified, Smoothed, SparseVolume,  # noqa: F401
                   align_volume, color_mesh,
                   component_stats, cube_axis, cube_points, eikonal_residual,
                   extract_mesh_sparse, extract_mesh_with_marching_cubes, keep_components,
                   label_components, marching_cubes, mesh_boundary, mesh_components, normal_mesh,
                   sdf_cube, shade_surface, simplify_grid, simplify_mesh, smooth_lattice,
                   smooth_mesh, sparse_extract, sparse_mesh, world_to_network, xyz2mesh)
from .raster import (Raster, interpolate_vertex_attributes, load_obj, rasterize_mesh,  # noqa: F401
                     render_mesh, subdivide_mesh)
from .options import AttrDict, SDFOptions, vol_render_opt  # noqa: F401
from . import training  # noqa: F401  (stage-2 DDP trainer, Discriminator, losses)
from .renderer import (FCGenerator, FiLMSiren, Geometry, LinearLayer,  # noqa: F401
                       NGPSIRENGenerator, SirenGenerator, Surface, VolumeFeatureRenderer,
                       get_encoder)

__version__ = "0.1.0"
