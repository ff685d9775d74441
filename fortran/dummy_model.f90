!===============================================================================
! dummy_model -- a RUNNABLE counterpart of the reference's outline program
! (ref: generic/dummy_model.f90:24-56, "not intended to work"): the same call order
!
!     atmos_step:  get_edges -> get_dist -> physics -> seabreeze_diag
!
! on the field layout of get_all_fields_mod (ref: generic/get_all_fields_mod.f90:9-19),
! linked against the drop-in modules of this directory, i.e. against libseabreeze_hip.so.
! BASELINE.json configs[0]: a 96x72 synthetic coastline.
!
! Usage:  dummy_model <input.bin> <output.bin> <nsteps> [mode ...]
!   input.bin : nx ny nz halo (4 x int32), then REAL arrays in Fortran order:
!               lon(nx) lat(ny) land_frac(nx,ny) ice_frac(nx,ny) z(nx,ny) sigma(nx,ny)
!               p(nx,ny,nz), then per step: theta(nx,ny) u(nx,ny,nz) v(nx,ny,nz)
!   output.bin: cdist(nx,ny), then per step: sb_con windspeed winddir thc (nx,ny each)
!   mode (optional):
!     status                     the argument checks of seabreeze_diag_status / seabreeze_diag_um (error = 1 for
!                                inconsistent shapes, before any device work: runs without a GPU)
!     um                         the Unified Model hook's argument order and bounds (seabreeze_diag_um) on the
!                                sub-domain the rim of the input fields leaves
!     um2d                       the UM copy's whole chain on the sub-domain of `um`: get_edges_um -> get_dist_um
!                                (window +-(halo_size + 3) cells, 2-D coordinates: the broadcast of lon and lat)
!                                -> seabreeze_diag_um; output.bin: the distance field on tdims_l (its ghost cells
!                                the edge cells, filled here), then per step sb_con windspeed winddir thc
!     um2dice                    um2d's sub-domain with sea ice that differs from step to step, as the UM rebuilds its mask
!                                from icefrac inside the timestep routine: um_coast_open once, then um_ice ahead of
!                                every seabreeze_diag_um.  Step s ices (0.6) the sea cells of the sub-domain that touch
!                                land and whose row j has mod(j + s, 3) == 0.  output.bin: per step the distance field on
!                                tdims_l (ghost cells the edge cells, filled here), then sb_con windspeed winddir thc
!     umtile                     um2d's sub-domain cut into 2 x 2 tiles, as a host model on a 2-D decomposition holds it: every
!                                tile's frames (halo_size + 4 ghost cells) are copied out of the whole fields, in the role of
!                                swap_bounds; tile_get_edges_um (ext = the window) and tile_get_dist_um (window +-(halo_size
!                                + 3) cells) per tile, reassembled and compared with the whole-domain get_edges_um ->
!                                get_dist_um_win; prints the number of differing cells and the largest difference.  No steps
!                                are run; output.bin holds the whole-domain distance field (interior) and the reassembled one
!     umtileice                  umtile's cut with um2dice's sea ice: <nsteps> ice planes (no steps are run).  Per plane the
!                                whole-domain get_edges_um -> get_dist_um_win; per tile um_tile_coast_open once, then
!                                swap_bounds' copy of icefrac and um_tile_ice per plane, um_tile_ice_report,
!                                um_tile_coast_close; reassembled and compared plane by plane: prints the number of differing
!                                cells and the largest difference, and the reports summed over the tiles.  output.bin: per
!                                plane the whole-domain distance field (interior) and the reassembled one
!     host                       the reference's call shape: host arrays in, host arrays out (default)
!     dev                        the fields live on the device (sb_dev_alloc); per step only theta, u, v go up
!                                and the four outputs come back; seabreeze_diag_dev
!     band <rank> <nranks> <idfile>
!                                one process per GPU, this one owns latitude band <rank> of <nranks>: the
!                                RCCL id travels through <idfile> (a real host model would MPI_Bcast it),
!                                static fields get their ghost rows once through swap_bounds, every step is one
!                                band_seabreeze_diag; output.bin then holds this band's rows only
!                                (cdist(nx,nyl), then per step the four (nx,nyl) fields)
!     bandsetup                  the coast setup per latitude band: coast and distance of the grid with the whole-grid
!                                routines, then, in this process, of three bands in frames cut here
!                                (band_get_edges, band_get_dist); stops at the first cell that differs, prints
!                                "bandsetup ok" otherwise.  No steps are run, output.bin holds cdist only
!     radius                     search_radius: the window radius of every band cell of the grid (the whole-grid routine,
!                                periodic and clamped), then of three bands in frames of halo_size ghost cells cut here
!                                (band_search_radius): a band's cell must have the grid's radius where that is within
!                                reach of its ghost rows, -1 where it is not; stops at the first cell that violates
!                                this, prints "radius ok" otherwise.  No steps are run; output.bin holds cdist, then
!                                the grid's radius plane (nx,ny) as 32-bit integers
! The tests write input.bin with numpy and compare output.bin with the CPU oracle.
!
! Two deliberate differences from the outline, both documented in INTEGRATION.md:
!  * `physics` passes (theta, mask, z, sigma) in the order of seabreeze_diag's own dummies;
!    the outline permutes them (ref: generic/dummy_model.f90:52-54 vs
!    generic/sea_breeze_diag.f90:55-56, SURVEY.md App. C #4).
!  * the distance field, not the coast mask, is what seabreeze_diag receives as `mask`
!    (ref: generic/sea_breeze_diag.f90:76 "distance form the coast").
!===============================================================================
module model_fields
  implicit none
  integer :: nx, ny, nz, halo_size
  real :: timestep = 24*60.                  ! seconds
  integer :: timestep_number
  real, allocatable :: lon(:), lat(:)
  real, allocatable :: p(:,:,:), u(:,:,:), v(:,:,:)
  real, allocatable :: sb_con(:,:), land_frac(:,:), ice_frac(:,:), windspeed(:,:), winddir(:,:), thc(:,:)
  real, allocatable :: z(:,:), sigma(:,:), theta(:,:), cdist(:,:)
  real, allocatable :: mask(:,:)             ! coast mask with ghost cells, as get_edges writes it
end module model_fields

program dummy_model
  use iso_c_binding
  use model_fields
  implicit none
  character(len=512) :: fin, fout, arg, mode, idfile
  integer :: nsteps, step, uin, uout, rank, nranks
  integer(4) :: hdr(4)

  if (command_argument_count() < 3) then
    print *, 'usage: dummy_model <input.bin> <output.bin> <nsteps> [host | dev | um | um2d | um2dice | umtile | umtileice | status | bandsetup | radius | band <rank> <nranks> <idfile>]'
    error stop 2
  end if
  call get_command_argument(1, fin)
  call get_command_argument(2, fout)
  call get_command_argument(3, arg)
  read (arg, *) nsteps
  mode = 'host'
  if (command_argument_count() >= 4) call get_command_argument(4, mode)
  rank = 0; nranks = 1
  if (trim(mode) == 'band') then
    if (command_argument_count() < 7) error stop 'band mode needs <rank> <nranks> <idfile>'
    call get_command_argument(5, arg); read (arg, *) rank
    call get_command_argument(6, arg); read (arg, *) nranks
    call get_command_argument(7, idfile)
  end if

  open (newunit=uin, file=trim(fin), access='stream', form='unformatted', status='old')
  read (uin) hdr
  nx = hdr(1); ny = hdr(2); nz = hdr(3); halo_size = hdr(4)
  allocate(lon(nx), lat(ny), p(nx,ny,nz), u(nx,ny,nz), v(nx,ny,nz))
  allocate(sb_con(nx,ny), land_frac(nx,ny), ice_frac(nx,ny), windspeed(nx,ny), winddir(nx,ny), thc(nx,ny))
  allocate(z(nx,ny), sigma(nx,ny), theta(nx,ny), cdist(nx,ny))
  allocate(mask(nx+2*halo_size, ny+2*halo_size))
  read (uin) lon, lat, land_frac, ice_frac, z, sigma, p
  sb_con = 0.; windspeed = 0.; winddir = 0.; thc = 0.

  open (newunit=uout, file=trim(fout), access='stream', form='unformatted', status='replace')
  select case (trim(mode))
  case ('host')
    do step = 1, nsteps
      timestep_number = step
      read (uin) theta, u, v
      call atmos_step()
      if (step == 1) write (uout) cdist
      write (uout) sb_con, windspeed, winddir, thc
    end do
  case ('dev')
    call run_device_resident()
  case ('band')
    call run_band()
  case ('um')
    call run_um()
  case ('um2d')
    call run_um2d()
  case ('um2dice')
    call run_um2dice()
  case ('umtile')
    call run_umtile()
  case ('umtileice')
    call run_umtileice()
  case ('status')
    call check_status()
  case ('bandsetup')
    call run_band_setup()
  case ('radius')
    call run_radius()
  case default
    error stop 'unknown mode'
  end select
  close (uin); close (uout)
  print '(a,a,a,i0,a,i0,a,i0,a,es12.5)', 'dummy_model (', trim(mode), '): ', nsteps, ' steps on ', nx, 'x', ny, &
        ', sum(sb_con) = ', sum(sb_con)

contains

  subroutine atmos_step()
    use sea_breeze_diag_mod, only : get_edges, get_dist
    call get_edges(mask, ice_frac, land_frac, halo_size)
    call get_dist(mask, land_frac, lon, lat, 180, cdist, halo_size)
    call physics(p, u, v, theta, z, sigma, cdist, windspeed, winddir, thc, sb_con, timestep_number, timestep)
  end subroutine atmos_step

  subroutine physics(p, u, v, theta, z, sigma, mask, windspeed, winddir, thc, sb_con, timestep_number, timestep)
    use sea_breeze_diag_mod, only : seabreeze_diag
    real, intent(in), dimension(:,:,:) :: p, u, v
    real, intent(in), dimension(:,:) :: mask, theta, z, sigma
    real, intent(inout), dimension(:,:) :: thc, windspeed, winddir, sb_con
    real, intent(in) :: timestep
    integer, intent(in) :: timestep_number
    call seabreeze_diag(timestep, timestep_number, p, u, v, theta, mask, z, sigma, windspeed, winddir, thc, sb_con)
  end subroutine physics

  !---------------------------------------------------------------------------
  ! The coast setup band by band against the whole-grid routines: three bands of uneven height, each in a frame of
  ! halo_size ghost cells cut out of the global fields here (what swap_bounds delivers on a multi-rank run: the
  ! neighbours' rows on a cut side).  Ghost rows beyond a pole, their latitudes and the east-west ghost columns are
  ! NaN: they are never read.  The window is +-halo_size cells, as in atmos_step.
  !---------------------------------------------------------------------------
  subroutine run_band_setup()
    use, intrinsic :: ieee_arithmetic, only : ieee_value, ieee_quiet_nan
    use sea_breeze_diag_mod, only : get_edges, get_dist, band_get_edges, band_get_dist
    integer :: h, b, r0, r1, nyl, i, j, lo, hi, cuts(4)
    real :: nan
    real, allocatable :: lf(:,:), ic(:,:), cf(:,:), df(:,:), latf(:)
    h = halo_size
    nan = ieee_value(nan, ieee_quiet_nan)
    call get_edges(mask, ice_frac, land_frac, h)
    call get_dist(mask, land_frac, lon, lat, 180, cdist, h)
    write (uout) cdist
    cuts = [0, ny/3 - 1, 2*(ny/3) + 2, ny]
    if (cuts(2) < 1 .or. cuts(3) <= cuts(2) .or. cuts(3) >= ny) error stop 'bandsetup: grid too small for three bands'
    do b = 1, 3
      r0 = cuts(b); r1 = cuts(b+1); nyl = r1 - r0                ! rows r0+1 .. r1 (1-based) of the grid
      allocate(lf(nx+2*h, nyl+2*h), ic(nx+2*h, nyl+2*h), cf(nx+2*h, nyl+2*h), df(nx+2*h, nyl+2*h), latf(nyl+2*h))
      lf = nan; ic = nan; latf = nan; cf = -777.; df = -777.
      lo = max(r0 - h, 0); hi = min(r1 + h, ny)                  ! the grid rows lo+1 .. hi lie in the frame
      lf(1+h:nx+h, lo-r0+h+1:hi-r0+h) = land_frac(:, lo+1:hi)
      ic(1+h:nx+h, lo-r0+h+1:hi-r0+h) = ice_frac(:, lo+1:hi)
      latf(lo-r0+h+1:hi-r0+h) = lat(lo+1:hi)
      call band_get_edges(cf, ic, lf, h, b == 1, b == 3)
      do j = 1, nyl
        do i = 1, nx
          if (cf(i+h, j+h) /= mask(i+h, r0+j+h)) then
            print '(a,i0,a,i0,a,i0)', 'bandsetup: coast differs in band ', b, ' at ', i, ',', r0 + j
            error stop 'bandsetup: band_get_edges differs from get_edges'
          end if
        end do
      end do
      if (any(cf(:, :h) /= -777.) .or. any(cf(:, nyl+h+1:) /= -777.) .or. any(cf(:h, :) /= -777.) .or. &
          any(cf(nx+h+1:, :) /= -777.)) error stop 'bandsetup: band_get_edges wrote ghost cells'
      ! (the exchange of coast's ghost rows: the neighbours' rows of the whole-grid coast, which the bands reproduce)
      cf = nan
      cf(1+h:nx+h, lo-r0+h+1:hi-r0+h) = mask(1+h:nx+h, lo+1+h:hi+h)
      call band_get_dist(cf, lf, lon, latf, 180, df, h, b == 1, b == 3)
      do j = 1, nyl
        do i = 1, nx
          if (df(i+h, j+h) /= cdist(i, r0+j)) then
            print '(a,i0,a,i0,a,i0,2es24.16)', 'bandsetup: distance differs in band ', b, ' at ', i, ',', r0 + j, &
                  df(i+h, j+h), cdist(i, r0+j)
            error stop 'bandsetup: band_get_dist differs from get_dist'
          end if
        end do
      end do
      if (any(df(:, :h) /= -777.) .or. any(df(:, nyl+h+1:) /= -777.) .or. any(df(:h, :) /= -777.) .or. &
          any(df(nx+h+1:, :) /= -777.)) error stop 'bandsetup: band_get_dist wrote ghost cells'
      deallocate(lf, ic, cf, df, latf)
    end do
    print '(a)', 'bandsetup ok'
  end subroutine run_band_setup

  !---------------------------------------------------------------------------
  ! The window radii of the grid and of three bands of it (the cuts of run_band_setup), each band in a frame of
  ! halo_size ghost cells whose rows on a cut side are the neighbours' rows of the distance field (what swap_bounds
  ! delivers); ghost rows beyond a pole and the east-west ghost columns are NaN: they are never read.  A band's window
  ! may use its ghost rows and no more: reach = halo_size + the distance to the nearest cut side.
  !---------------------------------------------------------------------------
  subroutine run_radius()
    use, intrinsic :: ieee_arithmetic, only : ieee_value, ieee_quiet_nan
    use sea_breeze_diag_mod, only : get_edges, get_dist, search_radius, band_search_radius
    integer :: h, b, r0, r1, nyl, i, j, lo, hi, cuts(4), reach, want
    integer(c_int), allocatable :: rad(:,:), rb(:,:)
    integer(c_long_long) :: summ(4), sb(4)
    real :: nan
    real, allocatable :: mf(:,:)
    h = halo_size
    nan = ieee_value(nan, ieee_quiet_nan)
    call get_edges(mask, ice_frac, land_frac, h)
    call get_dist(mask, land_frac, lon, lat, 180, cdist, h)
    write (uout) cdist
    allocate(rad(nx, ny))
    call search_radius(cdist, 180., rad, summ, 0)
    if (summ(1) /= count(rad /= 0) .or. summ(2) /= count(rad > 0) .or. summ(3) /= count(rad == -1) .or. &
        summ(4) /= max(maxval(rad), 0)) error stop 'radius: summary does not describe the plane'
    cuts = [0, ny/3 - 1, 2*(ny/3) + 2, ny]
    if (cuts(2) < 1 .or. cuts(3) <= cuts(2) .or. cuts(3) >= ny) error stop 'radius: grid too small for three bands'
    do b = 1, 3
      r0 = cuts(b); r1 = cuts(b+1); nyl = r1 - r0                ! rows r0+1 .. r1 (1-based) of the grid
      allocate(mf(nx+2*h, nyl+2*h), rb(nx, nyl))
      mf = nan
      lo = max(r0 - h, 0); hi = min(r1 + h, ny)                  ! the grid rows lo+1 .. hi lie in the frame
      mf(1+h:nx+h, lo-r0+h+1:hi-r0+h) = cdist(:, lo+1:hi)
      call band_search_radius(mf, 180., rb, sb, h, b == 1, b == 3)
      do j = 1, nyl
        reach = huge(reach)
        if (b /= 1) reach = min(reach, j - 1 + h)
        if (b /= 3) reach = min(reach, nyl - j + h)
        do i = 1, nx
          want = rad(i, r0+j)
          if (want > reach) want = -1
          if (rb(i, j) /= want) then
            print '(a,i0,a,i0,a,i0,a,i0,a,i0)', 'radius: band ', b, ' differs at ', i, ',', r0 + j, ': ', rb(i, j), ' /= ', want
            error stop 'radius: band_search_radius violates the band property'
          end if
        end do
      end do
      if (sb(1) /= count(rb /= 0) .or. sb(3) /= count(rb == -1)) error stop 'radius: band summary does not describe the plane'
      deallocate(mf, rb)
    end do
    print '(a)', 'radius ok'
    write (uout) rad
  end subroutine run_radius

  !---------------------------------------------------------------------------
  ! fields resident on the device: static ones go up once, per step theta, u, v
  !---------------------------------------------------------------------------
  subroutine run_device_resident()
    use sea_breeze_diag_mod, only : get_edges, get_dist, seabreeze_diag_dev
    use sb_context_mod, only : sb_dev_alloc, sb_dev_free, sb_dev_upload, sb_dev_download
    type(c_ptr) :: d_p, d_u, d_v, d_th, d_mask, d_z, d_sg, d_ws, d_wd, d_thc, d_sb
    integer(c_size_t) :: b2, b3
    real, target, allocatable :: buf2(:,:), buf3(:,:,:)
    b2 = int(nx, c_size_t) * ny * (storage_size(theta) / 8)
    b3 = b2 * nz
    call get_edges(mask, ice_frac, land_frac, halo_size)
    call get_dist(mask, land_frac, lon, lat, 180, cdist, halo_size)
    write (uout) cdist
    d_p = sb_dev_alloc(b3); d_u = sb_dev_alloc(b3); d_v = sb_dev_alloc(b3)
    d_th = sb_dev_alloc(b2); d_mask = sb_dev_alloc(b2); d_z = sb_dev_alloc(b2); d_sg = sb_dev_alloc(b2)
    d_ws = sb_dev_alloc(b2); d_wd = sb_dev_alloc(b2); d_thc = sb_dev_alloc(b2); d_sb = sb_dev_alloc(b2)
    allocate(buf2(nx,ny), buf3(nx,ny,nz))
    buf3 = p;      call sb_dev_upload(d_p, c_loc(buf3), b3)
    buf2 = cdist;  call sb_dev_upload(d_mask, c_loc(buf2), b2)
    buf2 = z;      call sb_dev_upload(d_z, c_loc(buf2), b2)
    buf2 = sigma;  call sb_dev_upload(d_sg, c_loc(buf2), b2)
    buf2 = 0.
    call sb_dev_upload(d_ws, c_loc(buf2), b2); call sb_dev_upload(d_wd, c_loc(buf2), b2)
    call sb_dev_upload(d_thc, c_loc(buf2), b2); call sb_dev_upload(d_sb, c_loc(buf2), b2)
    do step = 1, nsteps
      read (uin) theta, u, v
      buf2 = theta; call sb_dev_upload(d_th, c_loc(buf2), b2)
      buf3 = u;     call sb_dev_upload(d_u, c_loc(buf3), b3)
      buf3 = v;     call sb_dev_upload(d_v, c_loc(buf3), b3)
      call seabreeze_diag_dev(timestep, step, nx, ny, nz, 0, d_p, d_u, d_v, d_th, d_mask, d_z, d_sg, &
                              d_ws, d_wd, d_thc, d_sb)
      call sb_dev_download(c_loc(buf2), d_sb, b2);  sb_con = buf2
      call sb_dev_download(c_loc(buf2), d_ws, b2);  windspeed = buf2
      call sb_dev_download(c_loc(buf2), d_wd, b2);  winddir = buf2
      call sb_dev_download(c_loc(buf2), d_thc, b2); thc = buf2
      write (uout) sb_con, windspeed, winddir, thc
    end do
    call sb_dev_free(d_p); call sb_dev_free(d_u); call sb_dev_free(d_v); call sb_dev_free(d_th)
    call sb_dev_free(d_mask); call sb_dev_free(d_z); call sb_dev_free(d_sg)
    call sb_dev_free(d_ws); call sb_dev_free(d_wd); call sb_dev_free(d_thc); call sb_dev_free(d_sb)
  end subroutine run_device_resident

  !---------------------------------------------------------------------------
  ! The Unified Model hook's argument list and bounds (ref: UM/vn10.7/sea_breeze_diag.F90:55-56,66-117):
  ! the rim of the input fields serves as the ghost cells of a sub-domain -- theta, z, sigma with a small
  ! halo of halo_size + 1 cells (the widest window of a coastal-band cell), the coast distance with a large
  ! halo of halo_size + 3 -- and the diagnostic is called with (theta, z, sigma, mask) in the UM's order and
  ! its `error` status.  Output: the sub-domain's fields, per step.
  !---------------------------------------------------------------------------
  subroutine run_um()
    use sea_breeze_diag_mod, only : get_edges, get_dist, seabreeze_diag_um
    integer :: hs, hl, nxi, nyi, error
    real, allocatable :: p_i(:,:,:), u_i(:,:,:), v_i(:,:,:), th_s(:,:), z_s(:,:), sg_s(:,:)
    real, allocatable :: ws_i(:,:), wd_i(:,:), thc_i(:,:), sb_i(:,:)
    hs = halo_size + 1; hl = halo_size + 3
    nxi = nx - 2*hl; nyi = ny - 2*hl
    if (nxi < 1 .or. nyi < 1) error stop 'um mode: grid too small for the ghost frame'
    call get_edges(mask, ice_frac, land_frac, halo_size)
    call get_dist(mask, land_frac, lon, lat, 180, cdist, halo_size)
    write (uout) cdist
    allocate(p_i(nxi,nyi,nz), u_i(nxi,nyi,nz), v_i(nxi,nyi,nz))
    allocate(th_s(nxi+2*hs,nyi+2*hs), z_s(nxi+2*hs,nyi+2*hs), sg_s(nxi+2*hs,nyi+2*hs))
    allocate(ws_i(nxi,nyi), wd_i(nxi,nyi), thc_i(nxi,nyi), sb_i(nxi,nyi))
    ws_i = 0.; wd_i = 0.; thc_i = 0.; sb_i = 0.
    p_i = p(1+hl:nx-hl, 1+hl:ny-hl, :)
    z_s = z(1+hl-hs:nx-hl+hs, 1+hl-hs:ny-hl+hs)
    sg_s = sigma(1+hl-hs:nx-hl+hs, 1+hl-hs:ny-hl+hs)
    do step = 1, nsteps
      read (uin) theta, u, v
      u_i = u(1+hl:nx-hl, 1+hl:ny-hl, :)
      v_i = v(1+hl:nx-hl, 1+hl:ny-hl, :)
      th_s = theta(1+hl-hs:nx-hl+hs, 1+hl-hs:ny-hl+hs)
      call seabreeze_diag_um(timestep, step, p_i, u_i, v_i, th_s, z_s, sg_s, cdist, ws_i, wd_i, thc_i, sb_i, error)
      if (error /= 0) error stop 'um mode: seabreeze_diag_um reported an error'
      write (uout) sb_i, ws_i, wd_i, thc_i, th_s
    end do
    sb_con = 0.
    sb_con(1+hl:nx-hl, 1+hl:ny-hl) = sb_i
  end subroutine run_um

  !---------------------------------------------------------------------------
  ! The UM copy's setup and diagnostic on the sub-domain of run_um: coordinates as 2-D fields (here the
  ! broadcast of the input's 1-D lon, lat; a rotated-pole grid passes its true_latitude, true_longitude),
  ! get_edges_um (ref: UM/vn10.7/sea_breeze_diag.F90:328-446) and get_dist_um (:448-601) with a window of
  ! +-hl cells, the distance field's ghost cells filled by edge replication (standing in for swap_bounds at a
  ! limited-area edge), then seabreeze_diag_um every step.
  !---------------------------------------------------------------------------
  subroutine run_um2d()
    use sea_breeze_diag_mod, only : get_edges_um, get_dist_um, seabreeze_diag_um
    integer :: hs, hl, nxi, nyi, error, i, j
    real, allocatable :: p_i(:,:,:), u_i(:,:,:), v_i(:,:,:), th_s(:,:), z_s(:,:), sg_s(:,:)
    real, allocatable :: ws_i(:,:), wd_i(:,:), thc_i(:,:), sb_i(:,:), lf_i(:,:), ci_i(:,:)
    real, allocatable :: tlat(:,:), tlon(:,:), coast_l(:,:)
    hs = halo_size + 1; hl = halo_size + 3
    nxi = nx - 2*hl; nyi = ny - 2*hl
    if (nxi < 1 .or. nyi < 1) error stop 'um2d mode: grid too small for the ghost frame'
    allocate(lf_i(nxi,nyi), ci_i(nxi,nyi), tlat(nxi,nyi), tlon(nxi,nyi), coast_l(nxi+2*hl,nyi+2*hl))
    lf_i = land_frac(1+hl:nx-hl, 1+hl:ny-hl)
    ci_i = ice_frac(1+hl:nx-hl, 1+hl:ny-hl)
    do j = 1, nyi
      tlon(:, j) = lon(1+hl:nx-hl)
    end do
    do i = 1, nxi
      tlat(i, :) = lat(1+hl:ny-hl)
    end do
    coast_l = 0.
    call get_edges_um(coast_l, ci_i, lf_i)
    call get_dist_um(lf_i, coast_l, tlat, tlon)
    do j = 1, nyi + 2*hl                         ! ghost cells: the edge cells
      do i = 1, nxi + 2*hl
        coast_l(i, j) = coast_l(min(max(i, 1+hl), nxi+hl), min(max(j, 1+hl), nyi+hl))
      end do
    end do
    write (uout) coast_l
    allocate(p_i(nxi,nyi,nz), u_i(nxi,nyi,nz), v_i(nxi,nyi,nz))
    allocate(th_s(nxi+2*hs,nyi+2*hs), z_s(nxi+2*hs,nyi+2*hs), sg_s(nxi+2*hs,nyi+2*hs))
    allocate(ws_i(nxi,nyi), wd_i(nxi,nyi), thc_i(nxi,nyi), sb_i(nxi,nyi))
    ws_i = 0.; wd_i = 0.; thc_i = 0.; sb_i = 0.
    p_i = p(1+hl:nx-hl, 1+hl:ny-hl, :)
    z_s = z(1+hl-hs:nx-hl+hs, 1+hl-hs:ny-hl+hs)
    sg_s = sigma(1+hl-hs:nx-hl+hs, 1+hl-hs:ny-hl+hs)
    do step = 1, nsteps
      read (uin) theta, u, v
      u_i = u(1+hl:nx-hl, 1+hl:ny-hl, :)
      v_i = v(1+hl:nx-hl, 1+hl:ny-hl, :)
      th_s = theta(1+hl-hs:nx-hl+hs, 1+hl-hs:ny-hl+hs)
      call seabreeze_diag_um(timestep, step, p_i, u_i, v_i, th_s, z_s, sg_s, coast_l, ws_i, wd_i, thc_i, sb_i, error)
      if (error /= 0) error stop 'um2d mode: seabreeze_diag_um reported an error'
      write (uout) sb_i, ws_i, wd_i, thc_i
    end do
    sb_con = 0.
    sb_con(1+hl:nx-hl, 1+hl:ny-hl) = sb_i
  end subroutine run_um2d

  !---------------------------------------------------------------------------
  ! um2d with a coast that follows the sea ice: the sub-domain, coordinates and window of run_um2d; landfrac and
  ! icefrac on tdims_l with their ghost cells the edge cells; um_ice ahead of every step's seabreeze_diag_um -- the
  ! first call computes the whole interior, later ones what the moved coast can reach.  The interior of cdist_l is left
  ! alone between the calls: the diagnostic gets a copy whose ghost cells are filled by edge replication.
  !---------------------------------------------------------------------------
  subroutine run_um2dice()
    use sea_breeze_diag_mod, only : um_coast_open, um_ice, um_ice_report, um_coast_close, seabreeze_diag_um
    integer :: hs, hl, nxi, nyi, error, i, j, ii, jj
    integer(c_long_long) :: rep(4)
    real, allocatable :: p_i(:,:,:), u_i(:,:,:), v_i(:,:,:), th_s(:,:), z_s(:,:), sg_s(:,:)
    real, allocatable :: ws_i(:,:), wd_i(:,:), thc_i(:,:), sb_i(:,:), lf_i(:,:), ci_i(:,:)
    real, allocatable :: tlat(:,:), tlon(:,:), lf_l(:,:), ci_l(:,:), cdist_l(:,:), mask_l(:,:)
    logical, allocatable :: shore(:,:)
    hs = halo_size + 1; hl = halo_size + 3
    nxi = nx - 2*hl; nyi = ny - 2*hl
    if (nxi < 1 .or. nyi < 1) error stop 'um2dice mode: grid too small for the ghost frame'
    allocate(lf_i(nxi,nyi), ci_i(nxi,nyi), tlat(nxi,nyi), tlon(nxi,nyi), shore(nxi,nyi))
    allocate(lf_l(nxi+2*hl,nyi+2*hl), ci_l(nxi+2*hl,nyi+2*hl), cdist_l(nxi+2*hl,nyi+2*hl), mask_l(nxi+2*hl,nyi+2*hl))
    lf_i = land_frac(1+hl:nx-hl, 1+hl:ny-hl)
    do j = 1, nyi
      tlon(:, j) = lon(1+hl:nx-hl)
    end do
    do i = 1, nxi
      tlat(i, :) = lat(1+hl:ny-hl)
    end do
    do j = 1, nyi                                ! sea cells that touch land
      do i = 1, nxi
        shore(i, j) = lf_i(i, j) == 0. .and. any(lf_i(max(i-1,1):min(i+1,nxi), max(j-1,1):min(j+1,nyi)) > 0.)
      end do
    end do
    do jj = 1, nyi + 2*hl
      do ii = 1, nxi + 2*hl
        lf_l(ii, jj) = lf_i(min(max(ii - hl, 1), nxi), min(max(jj - hl, 1), nyi))
      end do
    end do
    cdist_l = 0.
    call um_coast_open(tlat, tlon, hl, hl, hl, hl)
    allocate(p_i(nxi,nyi,nz), u_i(nxi,nyi,nz), v_i(nxi,nyi,nz))
    allocate(th_s(nxi+2*hs,nyi+2*hs), z_s(nxi+2*hs,nyi+2*hs), sg_s(nxi+2*hs,nyi+2*hs))
    allocate(ws_i(nxi,nyi), wd_i(nxi,nyi), thc_i(nxi,nyi), sb_i(nxi,nyi))
    ws_i = 0.; wd_i = 0.; thc_i = 0.; sb_i = 0.
    p_i = p(1+hl:nx-hl, 1+hl:ny-hl, :)
    z_s = z(1+hl-hs:nx-hl+hs, 1+hl-hs:ny-hl+hs)
    sg_s = sigma(1+hl-hs:nx-hl+hs, 1+hl-hs:ny-hl+hs)
    do step = 1, nsteps
      read (uin) theta, u, v
      ci_i = ice_frac(1+hl:nx-hl, 1+hl:ny-hl)
      do j = 1, nyi
        if (mod(j + step, 3) == 0) then
          where (shore(:, j)) ci_i(:, j) = 0.6
        end if
      end do
      do jj = 1, nyi + 2*hl
        do ii = 1, nxi + 2*hl
          ci_l(ii, jj) = ci_i(min(max(ii - hl, 1), nxi), min(max(jj - hl, 1), nyi))
        end do
      end do
      call um_ice(lf_l, ci_l, cdist_l)
      do jj = 1, nyi + 2*hl                      ! ghost cells: the edge cells
        do ii = 1, nxi + 2*hl
          mask_l(ii, jj) = cdist_l(min(max(ii, 1+hl), nxi+hl), min(max(jj, 1+hl), nyi+hl))
        end do
      end do
      u_i = u(1+hl:nx-hl, 1+hl:ny-hl, :)
      v_i = v(1+hl:nx-hl, 1+hl:ny-hl, :)
      th_s = theta(1+hl-hs:nx-hl+hs, 1+hl-hs:ny-hl+hs)
      call seabreeze_diag_um(timestep, step, p_i, u_i, v_i, th_s, z_s, sg_s, mask_l, ws_i, wd_i, thc_i, sb_i, error)
      if (error /= 0) error stop 'um2dice mode: seabreeze_diag_um reported an error'
      write (uout) mask_l, sb_i, ws_i, wd_i, thc_i
    end do
    call um_ice_report(rep)
    print '(a,4(1x,i0))', 'um2dice: ice report', rep
    call um_coast_close()
    sb_con = 0.
    sb_con(1+hl:nx-hl, 1+hl:ny-hl) = sb_i
  end subroutine run_um2dice

  !---------------------------------------------------------------------------
  ! The UM-layout coast setup on a 2-D decomposition: the sub-domain and coordinates of run_um2d, window +-hl cells.  The
  ! whole-domain pair runs on a layout of hl + 1 ghost cells (so that get_dist_um_win takes the kernel the tile call shares:
  ! the fields are then equal to the last bit).  The domain is cut 2 x 2; a tile's frames of ht = hl + 1 ghost cells are
  ! copied from the whole fields -- a neighbour's cells where the domain goes on, the edge cells beyond the domain's edge, as
  ! get_edges_um pads them -- which is what swap_bounds leaves on a real run.  Every rank then forms the coast of its interior
  ! and of the hl ghost cells its window reads, and the distance of its interior.
  !---------------------------------------------------------------------------
  subroutine run_umtile()
    use sea_breeze_diag_mod, only : get_edges_um, get_dist_um_win, tile_get_edges_um, tile_get_dist_um, &
                                    SB_TILE_WEST, SB_TILE_EAST, SB_TILE_SOUTH, SB_TILE_NORTH
    integer :: hl, ht, nxi, nyi, i, j, ti, tj, x0, x1, y0, y1, nxt, nyt, sides, gi, gj, ndiff
    integer :: xcut(3), ycut(3)
    real :: dmax
    real, allocatable :: lf_i(:,:), ci_i(:,:), tlat(:,:), tlon(:,:), whole_l(:,:), tiled(:,:)
    real, allocatable :: lf_t(:,:), ci_t(:,:), lat_t(:,:), lon_t(:,:), coast_t(:,:)
    hl = halo_size + 3; ht = hl + 1
    nxi = nx - 2*hl; nyi = ny - 2*hl
    if (nxi < 2 .or. nyi < 2) error stop 'umtile mode: grid too small for the ghost frame'
    allocate(lf_i(nxi,nyi), ci_i(nxi,nyi), tlat(nxi,nyi), tlon(nxi,nyi), whole_l(nxi+2*ht,nyi+2*ht), tiled(nxi,nyi))
    lf_i = land_frac(1+hl:nx-hl, 1+hl:ny-hl)
    ci_i = ice_frac(1+hl:nx-hl, 1+hl:ny-hl)
    do j = 1, nyi
      tlon(:, j) = lon(1+hl:nx-hl)
    end do
    do i = 1, nxi
      tlat(i, :) = lat(1+hl:ny-hl)
    end do
    whole_l = 0.
    call get_edges_um(whole_l, ci_i, lf_i)
    call get_dist_um_win(lf_i, whole_l, tlat, tlon, hl, hl)
    xcut = [0, nxi/2, nxi]; ycut = [0, nyi/2, nyi]
    tiled = -1.
    do tj = 1, 2
      do ti = 1, 2
        x0 = xcut(ti); x1 = xcut(ti+1); y0 = ycut(tj); y1 = ycut(tj+1)
        nxt = x1 - x0; nyt = y1 - y0
        sides = 0
        if (ti == 1) sides = sides + SB_TILE_WEST
        if (ti == 2) sides = sides + SB_TILE_EAST
        if (tj == 1) sides = sides + SB_TILE_SOUTH
        if (tj == 2) sides = sides + SB_TILE_NORTH
        allocate(lf_t(nxt+2*ht,nyt+2*ht), ci_t(nxt+2*ht,nyt+2*ht), lat_t(nxt+2*ht,nyt+2*ht), lon_t(nxt+2*ht,nyt+2*ht))
        allocate(coast_t(nxt+2*ht,nyt+2*ht))
        do j = 1, nyt + 2*ht                       ! in the role of swap_bounds
          do i = 1, nxt + 2*ht
            gi = min(max(x0 + i - ht, 1), nxi); gj = min(max(y0 + j - ht, 1), nyi)
            lf_t(i, j) = lf_i(gi, gj); ci_t(i, j) = ci_i(gi, gj)
            lat_t(i, j) = tlat(gi, gj); lon_t(i, j) = tlon(gi, gj)
          end do
        end do
        coast_t = 0.
        call tile_get_edges_um(lf_t, ci_t, coast_t, ht, ht, hl, hl, sides)
        call tile_get_dist_um(lf_t, coast_t, lat_t, lon_t, ht, ht, hl, hl, sides)
        tiled(x0+1:x1, y0+1:y1) = coast_t(1+ht:nxt+ht, 1+ht:nyt+ht)
        deallocate(lf_t, ci_t, lat_t, lon_t, coast_t)
      end do
    end do
    ndiff = count(tiled /= whole_l(1+ht:nxi+ht, 1+ht:nyi+ht))
    dmax = maxval(abs(tiled - whole_l(1+ht:nxi+ht, 1+ht:nyi+ht)))
    print '(a,1x,i0,1x,a,1x,es12.5)', 'umtile: differing cells', ndiff, 'largest difference', dmax
    write (uout) whole_l(1+ht:nxi+ht, 1+ht:nyi+ht), tiled
  end subroutine run_umtile

  !---------------------------------------------------------------------------
  ! A tile that follows moving sea ice: run_umtile's sub-domain, coordinates, window (+-hl), cut and frames (ht = hl + 1
  ! ghost cells, copied from the whole fields in the role of swap_bounds: the edge cells beyond the domain's edge, which is
  ! what the whole-domain get_edges_um holds in its ring) under run_um2dice's ice planes.  What a UM rank does per
  ! timestep: one swap_bounds of icefrac -- the copy below -- then um_tile_ice.  The module holds one context, so the tiles
  ! take turns: each opens its coast, runs the planes in order and closes it.
  !---------------------------------------------------------------------------
  subroutine run_umtileice()
    use sea_breeze_diag_mod, only : get_edges_um, get_dist_um_win, um_tile_coast_open, um_tile_ice, um_tile_ice_report, &
                                    um_tile_coast_close
    integer :: hl, ht, nxi, nyi, i, j, ti, tj, x0, x1, y0, y1, nxt, nyt, gi, gj, ndiff, s
    integer :: xcut(3), ycut(3), beyond(4)
    integer(c_long_long) :: rep(4), total(4)
    real :: dmax
    real, allocatable :: lf_i(:,:), ci_s(:,:,:), tlat(:,:), tlon(:,:), whole_l(:,:), whole(:,:,:), tiled(:,:,:)
    real, allocatable :: lf_t(:,:), ci_t(:,:), lat_t(:,:), lon_t(:,:), cd_t(:,:)
    logical, allocatable :: shore(:,:)
    hl = halo_size + 3; ht = hl + 1
    nxi = nx - 2*hl; nyi = ny - 2*hl
    if (nxi < 2 .or. nyi < 2) error stop 'umtileice mode: grid too small for the ghost frame'
    if (nsteps < 1) error stop 'umtileice mode: needs at least one ice plane'
    allocate(lf_i(nxi,nyi), ci_s(nxi,nyi,nsteps), tlat(nxi,nyi), tlon(nxi,nyi), whole_l(nxi+2*ht,nyi+2*ht), shore(nxi,nyi))
    allocate(whole(nxi,nyi,nsteps), tiled(nxi,nyi,nsteps))
    lf_i = land_frac(1+hl:nx-hl, 1+hl:ny-hl)
    do j = 1, nyi
      tlon(:, j) = lon(1+hl:nx-hl)
    end do
    do i = 1, nxi
      tlat(i, :) = lat(1+hl:ny-hl)
    end do
    do j = 1, nyi                                ! sea cells that touch land
      do i = 1, nxi
        shore(i, j) = lf_i(i, j) == 0. .and. any(lf_i(max(i-1,1):min(i+1,nxi), max(j-1,1):min(j+1,nyi)) > 0.)
      end do
    end do
    do s = 1, nsteps
      ci_s(:, :, s) = ice_frac(1+hl:nx-hl, 1+hl:ny-hl)
      do j = 1, nyi
        if (mod(j + s, 3) == 0) then
          where (shore(:, j)) ci_s(:, j, s) = 0.6
        end if
      end do
      whole_l = 0.
      call get_edges_um(whole_l, ci_s(:, :, s), lf_i)
      call get_dist_um_win(lf_i, whole_l, tlat, tlon, hl, hl)
      whole(:, :, s) = whole_l(1+ht:nxi+ht, 1+ht:nyi+ht)
    end do
    xcut = [0, nxi/2, nxi]; ycut = [0, nyi/2, nyi]
    tiled = -1.
    total = 0
    do tj = 1, 2
      do ti = 1, 2
        x0 = xcut(ti); x1 = xcut(ti+1); y0 = ycut(tj); y1 = ycut(tj+1)
        nxt = x1 - x0; nyt = y1 - y0
        beyond = [x0, nxi - x1, y0, nyi - y1]
        allocate(lf_t(nxt+2*ht,nyt+2*ht), ci_t(nxt+2*ht,nyt+2*ht), lat_t(nxt+2*ht,nyt+2*ht), lon_t(nxt+2*ht,nyt+2*ht))
        allocate(cd_t(nxt+2*ht,nyt+2*ht))
        do j = 1, nyt + 2*ht
          do i = 1, nxt + 2*ht
            gi = min(max(x0 + i - ht, 1), nxi); gj = min(max(y0 + j - ht, 1), nyi)
            lf_t(i, j) = lf_i(gi, gj)
            lat_t(i, j) = tlat(gi, gj); lon_t(i, j) = tlon(gi, gj)
          end do
        end do
        cd_t = 0.
        call um_tile_coast_open(lat_t, lon_t, ht, ht, hl, hl, beyond)
        do s = 1, nsteps
          do j = 1, nyt + 2*ht                     ! in the role of swap_bounds
            do i = 1, nxt + 2*ht
              gi = min(max(x0 + i - ht, 1), nxi); gj = min(max(y0 + j - ht, 1), nyi)
              ci_t(i, j) = ci_s(gi, gj, s)
            end do
          end do
          call um_tile_ice(lf_t, ci_t, cd_t)
          tiled(x0+1:x1, y0+1:y1, s) = cd_t(1+ht:nxt+ht, 1+ht:nyt+ht)
        end do
        call um_tile_ice_report(rep)
        total = total + rep
        call um_tile_coast_close()
        deallocate(lf_t, ci_t, lat_t, lon_t, cd_t)
      end do
    end do
    ndiff = count(tiled /= whole)
    dmax = maxval(abs(tiled - whole))
    print '(a,1x,i0,1x,a,1x,es12.5)', 'umtileice: differing cells', ndiff, 'largest difference', dmax
    print '(a,4(1x,i0))', 'umtileice: ice report', total
    do s = 1, nsteps
      write (uout) whole(:, :, s), tiled(:, :, s)
    end do
  end subroutine run_umtileice

  !---------------------------------------------------------------------------
  ! Argument checks of the status-returning entry points: they answer error = 1 before any device work
  ! (ref: UM/vn10.7/sea_breeze_diag.F90:102,198-202), so this mode runs without a GPU as well.
  !---------------------------------------------------------------------------
  subroutine check_status()
    use sea_breeze_diag_mod, only : seabreeze_diag_status, seabreeze_diag_um
    real, allocatable :: th_big(:,:), mk_big(:,:), ws_small(:,:), mk_small(:,:), th_s(:,:), z_s(:,:), sg_s(:,:)
    integer :: e_mixed, e_state, e_um
    u = 0.; v = 0.; theta = 280.; cdist = 0.
    ! the outline's own declaration: mask, theta (nx+halo_size, ny+halo_size) beside z, sigma (nx, ny)
    ! (ref: generic/get_all_fields_mod.f90:17-19)
    allocate(th_big(nx+halo_size, ny+halo_size), mk_big(nx+halo_size, ny+halo_size))
    th_big = 280.; mk_big = 0.
    call seabreeze_diag_status(timestep, 1, p, u, v, th_big, mk_big, z, sigma, windspeed, winddir, thc, sb_con, e_mixed)
    ! a state field of another shape than p's horizontal extent
    allocate(ws_small(nx-1, ny)); ws_small = 0.
    call seabreeze_diag_status(timestep, 1, p, u, v, theta, cdist, z, sigma, ws_small, winddir, thc, sb_con, e_state)
    ! UM bounds: the large halo (mask) must not be narrower than the small one (theta, z, sigma)
    allocate(th_s(nx+4, ny+4), z_s(nx+4, ny+4), sg_s(nx+4, ny+4), mk_small(nx+2, ny+2))
    th_s = 280.; z_s = 0.; sg_s = 1.; mk_small = 0.
    call seabreeze_diag_um(timestep, 1, p, u, v, th_s, z_s, sg_s, mk_small, windspeed, winddir, thc, sb_con, e_um)
    print '(a,3(1x,i0))', 'status:', e_mixed, e_state, e_um
    write (uout) real(e_mixed), real(e_state), real(e_um)
  end subroutine check_status

  !---------------------------------------------------------------------------
  ! one latitude band of a multi-GPU run
  !---------------------------------------------------------------------------
  subroutine run_band()
    use sea_breeze_diag_mod, only : get_edges, get_dist, band_seabreeze_diag
    use halo_exchange_mod, only : swap_bounds
    use sb_context_mod, only : sb_comm_get_unique_id, sb_comm_init, sb_comm_finalize, sb_last_step_report
    integer(c_signed_char) :: id(128)
    integer :: n_launch, n_rccl, n_group, n_copy
    integer :: r0, r1, nyl, h, base, rem, uid, ios, tries
    real, allocatable :: th_b(:,:), mask_b(:,:), z_b(:,:), sg_b(:,:)
    real, allocatable :: p_b(:,:,:), u_b(:,:,:), v_b(:,:,:)
    real, allocatable :: ws_b(:,:), wd_b(:,:), thc_b(:,:), sb_b(:,:)
    logical :: there

    ! get_dist looks +-halo_size cells around every coast cell, so a band cell can be halo_size + 1 cells from
    ! the nearest cell of the other class: that is the ghost width the contrast window needs
    h = halo_size + 1
    ! the setup chain works on the global static fields and runs before the communicator exists
    ! (swap_bounds inside get_edges is then the single-domain fill)
    call get_edges(mask, ice_frac, land_frac, halo_size)
    call get_dist(mask, land_frac, lon, lat, 180, cdist, halo_size)
    ! the RCCL id: rank 0 makes it, the others wait for the file
    if (rank == 0) then
      call sb_comm_get_unique_id(id)
      open (newunit=uid, file=trim(idfile)//'.tmp', access='stream', form='unformatted', status='replace')
      write (uid) id
      close (uid)
      call rename(trim(idfile)//'.tmp', trim(idfile))
    else
      do tries = 1, 6000
        inquire (file=trim(idfile), exist=there)
        if (there) exit
        call sleep_ms(10)
      end do
      if (.not. there) error stop 'band mode: the id file never appeared'
      open (newunit=uid, file=trim(idfile), access='stream', form='unformatted', status='old', iostat=ios)
      read (uid) id
      close (uid)
    end if
    call sb_comm_init(id, rank, nranks)
    ! contiguous, near-equal bands
    base = ny / nranks; rem = mod(ny, nranks)
    r0 = rank * base + min(rank, rem) + 1
    nyl = base + merge(1, 0, rank < rem)
    r1 = r0 + nyl - 1
    allocate(th_b(nx+2*h, nyl+2*h), mask_b(nx+2*h, nyl+2*h), z_b(nx+2*h, nyl+2*h), sg_b(nx+2*h, nyl+2*h))
    allocate(p_b(nx,nyl,nz), u_b(nx,nyl,nz), v_b(nx,nyl,nz))
    allocate(ws_b(nx,nyl), wd_b(nx,nyl), thc_b(nx,nyl), sb_b(nx,nyl))
    ws_b = 0.; wd_b = 0.; thc_b = 0.; sb_b = 0.
    mask_b = 0.; z_b = 0.; sg_b = 0.; th_b = 0.
    mask_b(1+h:nx+h, 1+h:nyl+h) = cdist(:, r0:r1)
    z_b(1+h:nx+h, 1+h:nyl+h) = z(:, r0:r1)
    sg_b(1+h:nx+h, 1+h:nyl+h) = sigma(:, r0:r1)
    ! static fields: ghost cells once (RCCL send/recv with the band neighbours, poles and E-W locally)
    call swap_bounds(mask_b, h)
    call swap_bounds(z_b, h)
    call swap_bounds(sg_b, h)
    p_b = p(:, r0:r1, :)
    write (uout) cdist(:, r0:r1)
    do step = 1, nsteps
      read (uin) theta, u, v
      th_b(1+h:nx+h, 1+h:nyl+h) = theta(:, r0:r1)
      u_b = u(:, r0:r1, :)
      v_b = v(:, r0:r1, :)
      call band_seabreeze_diag(timestep, step, p_b, u_b, v_b, th_b, mask_b, z_b, sg_b, ws_b, wd_b, thc_b, sb_b)
      write (uout) sb_b, ws_b, wd_b, thc_b
    end do
    sb_con = 0.
    sb_con(:, r0:r1) = sb_b
    call sb_last_step_report(n_launch, n_rccl, n_group, n_copy)
    print '(a,4(1x,i0))', 'band step enqueued (launches, RCCL ops, RCCL groups, copies):', n_launch, n_rccl, n_group, n_copy
    call sb_comm_finalize()
  end subroutine run_band

  subroutine sleep_ms(ms)
    integer, intent(in) :: ms
    integer(8) :: c0, c1, rate
    call system_clock(c0, rate)
    do
      call system_clock(c1)
      if ((c1 - c0) * 1000 >= int(ms, 8) * rate) exit
    end do
  end subroutine sleep_ms

end program dummy_model
